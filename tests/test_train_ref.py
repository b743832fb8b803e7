"""The float64 restatements of tests/train_ref.py against torch autograd in float64 (CPU only), at the shapes and input families
tests/test_hip_train_kernels.py uses: the arithmetic functions to 1e-12 relative, the pools exactly - ties, all-equal windows and
-inf inputs included, which proves the first-maximum rule is torch's."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import train_ref as TR

F64 = torch.float64
BF16, F32 = torch.bfloat16, torch.float32


def _close(a, b, what, rel=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{what}: not finite"
    d = float((a - b).abs().max())
    scale = float(b.abs().max())
    assert d <= rel * max(scale, 1e-300) or d == 0.0, f"{what}: {d:.3e} against {scale:.3e}"


@pytest.mark.parametrize("dtype,c", [(d, c) for d in (F32, BF16) for c in TR.BN_CHANNELS[d][:3]] + [(F32, 1024), (BF16, 2048)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_batchnorm_restatements_match_autograd(dtype, c):
    """bn_stats_ref / bn_act_fwd_ref / bn_act_bwd_ref against F.batch_norm(training=True) + F.silu differentiated in float64, on every
    case of the GPU file.  The comparison feeds the restatements the batch statistics themselves (what autograd differentiates
    through); every reference value is finite.  (The two widest channel counts walk the three smallest pixel counts and the largest.)"""
    for npix, family, act, _, with_res, running, seed in TR.bn_cases(dtype, c):
        if c >= 1024 and npix not in (1, 3, 63, 4099):
            continue
        z, dy, res, gamma, beta = TR.bn_family(family, npix, c, dtype, seed)
        what = f"{dtype} c{c} npix{npix} {family} act{act}"
        rm0, rv0 = torch.linspace(-0.1, 0.1, c, dtype=F64), torch.linspace(0.5, 1.5, c, dtype=F64)
        mean, var, run, A1, A2 = TR.bn_stats_ref(z, rm0, rv0, 0.03)
        zz = z.to(F64).t().reshape(1, c, npix).clone().requires_grad_(True)
        g64, b64 = gamma.to(F64).clone().requires_grad_(True), beta.to(F64).clone().requires_grad_(True)
        rm, rv = rm0.clone(), rv0.clone()
        if npix > 1:
            v = F.batch_norm(zz, rm, rv, g64, b64, True, TR.f32(0.03), TR.f32(TR.BN_EPS))
            _close(run[0], rm, what + " running mean")
            _close(run[1], rv, what + " running var")
        else:  # torch refuses one value per channel in training mode: the same normalisation spelt out
            v = (zz - zz.mean((0, 2), keepdim=True)) / torch.sqrt(zz.var((0, 2), unbiased=False, keepdim=True) + TR.f32(TR.BN_EPS))
            v = v * g64.view(1, c, 1) + b64.view(1, c, 1)
            _close(run[1], (1 - TR.f32(0.03)) * rv0 + TR.f32(0.03) * var, what + " running var at npix 1 (no n / (n - 1))")
        y = F.silu(v) if act == TR.ACT_SILU else v
        if with_res:
            y = y + res.to(F64).t().reshape(1, c, npix)
        y.backward(dy.to(F64).t().reshape(1, c, npix))
        _close(mean, zz.detach().mean((0, 2)), what + " mean")
        _close(var, zz.detach().var((0, 2), unbiased=False), what + " var", rel=1e-9 if family == "offset" else 1e-12)
        yr, My = TR.bn_act_fwd_ref(z, mean, var, gamma, beta, TR.BN_EPS, act, res if with_res else None)
        _close(yr, y.detach()[0].t(), what + " y")
        dz, dgamma, dbeta, Mdz, Sb, Sg, T, Tb, Tg = TR.bn_act_bwd_ref(z, dy, mean, var, gamma, beta, TR.BN_EPS, act)
        # autograd's dz cancels sum(du) and sum(du xhat) in its own order: absolute agreement relative to the magnitude term
        assert float(((dz - zz.grad[0].t()).abs() / (Mdz + 1e-300)).max()) <= 1e-9, what + " dz"
        assert float(((dgamma - g64.grad).abs() / (Sg + 1e-300)).max()) <= 1e-12, what + " dgamma"
        assert float(((dbeta - b64.grad).abs() / (Sb + 1e-300)).max()) <= 1e-12, what + " dbeta"
        for t in (yr, My, dz, Mdz, dgamma, dbeta, Sb, Sg, T, Tb, Tg, A1, A2):
            assert bool(torch.isfinite(t).all()), what


def test_c1_constants():
    """The constant c1 of the BatchNorm apply kernels' bound c1 2^-24 M: the worst |float32 restatement - float64 reference| / (2^-24 M)
    over every case of the GPU file, mean and var rounded to float32 as the kernels receive them; M = M_y forward, M_dz + T backward.
    (Against M_dz alone the backward figure is 1702: a SiLU derivative next to its zero leaves |du| a thousand times smaller than the
    |dy| its rounding error scales with - hence the term T, see bn_act_bwd_ref.)  train_ref.C1_FWD_CPU / C1_BWD_CPU
    record the measurement (rounded up); this test prints the figures and asserts that the record still covers them."""
    worst_f = worst_b = 0.0
    for dtype in (F32, BF16):
        for c in TR.BN_CHANNELS[dtype][:3]:
            for npix, family, act, _, with_res, _, seed in TR.bn_cases(dtype, c):
                z, dy, res, gamma, beta = TR.bn_family(family, npix, c, dtype, seed)
                mean, var = (t.float() for t in TR.bn_stats_ref(z)[:2])
                yr, My = TR.bn_act_fwd_ref(z, mean, var, gamma, beta, TR.BN_EPS, act, res if with_res else None)
                y32 = TR.bn_fwd_f32(z, mean, var, gamma, beta, TR.BN_EPS, act, res if with_res else None)
                worst_f = max(worst_f, float(((y32.to(F64) - yr).abs() / (TR.U24 * My + 1e-300)).max()))
                dz, dgamma, dbeta, Mdz, _, _, T, _, _ = TR.bn_act_bwd_ref(z, dy, mean, var, gamma, beta, TR.BN_EPS, act)
                d32 = TR.bn_bwd_f32(z, dy, mean, var, gamma, beta, TR.BN_EPS, act, dbeta, dgamma)
                worst_b = max(worst_b, float(((d32.to(F64) - dz).abs() / (TR.U24 * (Mdz + T) + 1e-300)).max()))
    print(f"c1 measured on the CPU: forward {worst_f:.3f}, backward {worst_b:.3f}")
    assert worst_f <= TR.C1_FWD_CPU and worst_b <= TR.C1_BWD_CPU, (worst_f, worst_b)
    assert TR.C1_FWD_CPU <= 1.25 * worst_f + 0.5 and TR.C1_BWD_CPU <= 1.25 * worst_b + 0.5, "the record is stale"


@pytest.mark.parametrize("cin,cout", TR.DGRAD_CHANNELS)
def test_dgrad_ref_matches_autograd(cin, cout):
    for hw in TR.DGRAD_MAPS:
        for dtype in (BF16, F32):
            x, dz, w = TR.conv_grad_family(2, cin, cout, hw[0], hw[1], 3, 2, 1, dtype, cin + hw[0])
            xr = x.to(F64).requires_grad_(True)
            F.conv2d(xr, w.to(F64), None, 2, 1).backward(dz.to(F64))
            dx, S = TR.dgrad_ref(dz, w, 2, 1, hw)
            _close(dx, xr.grad, f"dgrad {cin}->{cout} {hw}")
            assert bool((S + 1e-300 >= dx.abs()).all()) and bool(torch.isfinite(S).all())


def test_dgrad_ref_stride1_and_phase_weights():
    x, dz, w = TR.conv_grad_family(2, 8, 16, 7, 9, 3, 1, 1, F32, 5)
    xr = x.to(F64).requires_grad_(True)
    F.conv2d(xr, w.to(F64), None, 1, 1).backward(dz.to(F64))
    _close(TR.dgrad_ref(dz, w, 1, 1, (7, 9))[0], xr.grad, "dgrad stride 1")
    # the four phase kernels applied as the library applies them (k 2, pad 1 over dz, value of (i, j) at [i + 1][j + 1]) give dgrad_ref
    x, dz, w = TR.conv_grad_family(2, 8, 16, 7, 10, 3, 2, 1, F32, 6)
    v = TR.phase_weights_ref(w)  # [4][cin][cout][2][2]
    t = F.conv2d(dz.to(F64), v.reshape(4 * 8, 16, 2, 2).to(F64), None, 1, 1)
    dx = torch.zeros(2, 8, 7, 10, dtype=F64)
    for py in (0, 1):
        for px in (0, 1):
            ph = t[:, (2 * py + px) * 8:(2 * py + px + 1) * 8]
            sub = dx[:, :, py::2, px::2]
            sub.copy_(ph[:, :, 1:1 + sub.shape[2], 1:1 + sub.shape[3]])
    _close(dx, TR.dgrad_ref(dz, w, 2, 1, (7, 10))[0], "phases")


@pytest.mark.parametrize("case", TR.WGRAD_CASES, ids=[c[6].split(":")[0].replace(" ", "_") + f"_{c[1]}-{c[2]}" for c in TR.WGRAD_CASES])
def test_wgrad_ref_matches_autograd(case):
    dtype, cin, cout, k, s, p, _ = case
    n, h, w = TR.WGRAD_MAP
    x, dz, wt = TR.conv_grad_family(n, cin, cout, h, w, k, s, p, dtype, cin * 7 + cout)
    wr = wt.to(F64).requires_grad_(True)
    F.conv2d(x.to(F64), wr, None, s, p).backward(dz.to(F64))
    dw, S = TR.wgrad_ref(x, dz, k, s, p)
    _close(dw, wr.grad, str(case))
    assert bool((S + 1e-300 >= dw.abs()).all())


@pytest.mark.parametrize("ksp", TR.POOL_KSP, ids=lambda v: f"k{v[0]}s{v[1]}p{v[2]}")
def test_maxpool_bwd_ref_is_torch_exactly(ksp):
    k, s, p = ksp
    for (h, w) in TR.POOL_MAPS:
        if h + 2 * p < k or w + 2 * p < k:
            continue
        for family in TR.POOL_FAMILIES:
            for dtype in (F32, BF16):
                x, dy = TR.pool_family(family, 2, 8, h, w, k, s, p, dtype, h * 31 + w)
                xr = x.to(F64).requires_grad_(True)
                F.max_pool2d(xr, k, s, p).backward(dy.to(F64))
                dx, A = TR.maxpool_bwd_ref(x, dy, k, s, p)
                assert torch.equal(dx, xr.grad), f"{family} {ksp} {h}x{w}"
                assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(A).all())
                if family == "flat" and s == 1:  # only first taps are elected: the bottom-right pixel of a map larger than one window's reach gets nothing
                    assert float(dx[:, :, 0, 0].abs().min()) >= 0.0


def test_upsample_bwd_ref_is_torch_exactly():
    for (h, w) in ((1, 1), (5, 7)):
        dy = ((torch.rand(2, 8, 2 * h, 2 * w, generator=torch.Generator().manual_seed(h)) * 2 - 1) * 128).round() / 128
        u = torch.zeros(2, 8, h, w, dtype=F64, requires_grad=True)
        F.interpolate(u, scale_factor=2, mode="nearest").backward(dy.to(F64))
        dx, A = TR.upsample2x_bwd_ref(dy)
        assert torch.equal(dx, u.grad)


@pytest.mark.parametrize("n", [1, 1000])
def test_sgd_ref_matches_torch(n):
    """Three steps of clip_grad_norm_ + SGD(nesterov) + the EMA formula in float64 (state kept in float64 on both sides here: the
    rounding of the state to float32 between steps is the GPU test's business)."""
    g0 = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=g0, dtype=F64) * 2 - 1
    for wd in (5e-4, 0.0):
        pr = p.clone().requires_grad_(True)
        opt = torch.optim.SGD([pr], lr=TR.f32(0.01), momentum=TR.f32(0.9), nesterov=True, weight_decay=TR.f32(wd))
        P, B, E = p.clone(), torch.zeros(n, dtype=F64), p.clone()
        er = p.clone()
        for step in range(3):
            g = (torch.rand(n, generator=g0, dtype=F64) * 2 - 1) * (50.0 if step == 1 else 0.01)
            pr.grad = g.clone()
            total = float(g.norm())
            torch.nn.utils.clip_grad_norm_([pr], TR.f32(10.0))
            opt.step()
            d = TR.f32(0.9999 * (1 - math.exp(-(step + 1) / 2000.0)))
            er = er * d + (1 - d) * pr.detach()
            (P, G, B, E), _ = TR.sgd_ref(P, g, B, E, total * total, 10.0, 0.01, 0.9, wd, step == 0, d, 1)
            _close(P, pr.detach(), f"p step {step}", rel=1e-9)  # clip_grad_norm_'s 1e-6 is a float64 there, a float32 here
            _close(E, er, f"ema step {step}", rel=1e-9)
            assert float(G.abs().max()) == 0.0
    # a scaled step lands where the unscaled one does; an overflowing one moves the EMA only
    g = torch.rand(n, generator=g0, dtype=F64)
    ss = float((g * g).sum())
    a, _ = TR.sgd_ref(p, g, torch.zeros_like(p), p, ss, 10.0, 0.01, 0.9, 5e-4, True, 0.5, 0)
    b, _ = TR.sgd_ref(p, g * 1024.0, torch.zeros_like(p), p, ss * 1024.0 ** 2, 10.0, 0.01, 0.9, 5e-4, True, 0.5, 0, scale=1024.0)
    _close(b[0], a[0], "scaled p")
    c, _ = TR.sgd_ref(p, g, torch.ones_like(p), p * 2, math.inf, 10.0, 0.01, 0.9, 5e-4, False, 0.5, 1, scale=1024.0)
    assert torch.equal(c[0], p) and torch.equal(c[2], torch.ones_like(p)) and float(c[1].abs().max()) == 0.0
    _close(c[3], p * 2 * 0.5 + 0.5 * p, "ema of a skipped step")


def test_scaler_ref_matches_torch_gradscaler_rules():
    """torch/amp/grad_scaler.py update(): backoff and tracker reset on inf, growth after `interval` clean steps in a row."""
    st = [65536.0, 0.0, 0.0, 0.0]
    seq = [1.0, 2.0, math.inf, 1.0, 1.0, 1.0, math.nan, math.inf, 3.0]
    want = [(65536.0, 1), (65536.0, 2), (32768.0, 0), (32768.0, 1), (32768.0, 2), (65536.0, 0), (32768.0, 0), (16384.0, 0), (16384.0, 1)]
    for ss, (scale, tracker) in zip(seq, want):
        prev = st[0]
        st = TR.scaler_ref(st, ss, 2.0, 0.5, 3)
        assert st == [scale, float(tracker), 0.0 if math.isfinite(ss) else 1.0, prev]
