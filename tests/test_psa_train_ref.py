"""CPU: the float64 references and bounds of tests/psa_train_ref.py (the training forms of the PSA attention and the depthwise 3x3).

  * each reference equals float64 torch.autograd of the reference's own formulation (block.py:1701-1722 without pe; F.conv2d(groups=C))
    to 1e-12 relative;
  * a float32 emulation in three summation orders sits inside the bound on every case and family;
  * on `uniform` no bound exceeds 2^-6 max|ref| of its tensor (dq / dk of a single token are exactly zero and are left out);
  * each negative control is rejected by the bound on the case named beside it;
  * the entries refuse bad arguments on the host, and the trainers' remaining refusals."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import psa_train_ref as PR
from tests.yolo11_kernel_ref import CH, HD, KD, SCALE

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
FAMILIES = ["uniform", "positive", "impulse", "peaked"]
ATTN_CASES = [(1, 1, 1, 1), (2, 2, 2, 2), (1, 7, 7, 2), (1, 7, 9, 1), (1, 8, 8, 3), (1, 5, 13, 1), (1, 10, 13, 1)]  # (n, h, w, heads)
DW_CASES = [(1, 1, 1, 8), (1, 1, 5, 8), (3, 2, 2, 8), (1, 3, 7, 72), (2, 7, 7, 64)]  # (n, h, w, c)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _autograd_attention(qkv, d_o, heads, scale):
    """block.py:1713-1718: qkv.view(B, heads, 2 kd + hd, N).split -> attn = softmax(q^T k * scale) -> v @ attn^T, NCHW."""
    n, h, w, _ = qkv.shape
    N = h * w
    x = qkv.to(F64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    q, k, v = x.view(n, heads, CH, N).split([KD, KD, HD], dim=2)
    attn = ((q.transpose(-2, -1) @ k) * scale).softmax(dim=-1)
    o = (v @ attn.transpose(-2, -1)).view(n, heads * HD, h, w)
    (o * d_o.to(F64).permute(0, 3, 1, 2)).sum().backward()
    lse = torch.logsumexp((q.transpose(-2, -1) @ k) * scale, dim=-1).detach()
    return o.detach().permute(0, 2, 3, 1), lse, x.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=["x".join(map(str, c)) for c in ATTN_CASES])
def test_attention_references_bounds_and_f32_orders(case, family):
    n, h, w, heads = case
    scale = PR.f32_scale(SCALE)
    for dtype in (F32, BF16):
        qkv, d_o = PR.attn_inputs(family, n, h, w, heads, dtype)
        r = PR.attn_fwd_ref(qkv, heads, scale)
        o_a, lse_a, g_a = _autograd_attention(qkv, d_o, heads, scale)
        assert _rel(r["o"], o_a) <= 1e-12 and float((r["lse"] - lse_a).abs().max()) <= 1e-12 * max(1.0, float(lse_a.abs().max()))
        ref, bound = PR.attn_bwd_ref(qkv, r["o"], r["lse"], d_o, heads, scale, dtype)
        assert float((ref - g_a).abs().max()) <= 1e-12 * max(float(g_a.abs().max()), 1e-30)
        # the backward's inputs as the kernel gets them: o rounded to the storage type, lse to float32
        o_in, lse_in = r["o"].to(dtype).to(F64), r["lse"].float().to(F64)
        ref, bound = PR.attn_bwd_ref(qkv, o_in, lse_in, d_o, heads, scale, dtype)
        assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all())
        if family == "uniform":
            # (one token: dS = P (dp - D) is the difference of two equal dots, dq = dk = 0 exactly and only dv has a scale to compare with)
            for a, b, name in ((0, KD, "dq"), (KD, 2 * KD, "dk"), (2 * KD, CH, "dv"))[2 if h * w == 1 else 0:]:
                sl = lambda t: t.reshape(n, h, w, heads, CH)[..., a:b]  # noqa: E731
                assert float(sl(bound).max()) <= 2.0 ** -6 * float(sl(ref).abs().max()), (name, dtype)
        for order in ("natural", "reversed", "partitioned"):
            got = PR.attn_bwd_f32(qkv, o_in, lse_in, d_o, heads, scale, order)
            if dtype == BF16:
                got = got.to(BF16)
            err = (got.to(F64) - ref).abs()
            assert bool((err <= bound).all()), (order, dtype, float((err / bound).max()))
        # lse in float32, three orders of the channel dot
        q, k, _ = (t.float() for t in PR.psa_split(qkv, heads))
        for p in (torch.arange(KD), torch.arange(KD).flip(0), torch.arange(KD).roll(5)):
            s32 = (q * torch.tensor(scale, dtype=F32))[..., p] @ k[..., p].transpose(-1, -2)
            assert bool(((torch.logsumexp(s32, -1).to(F64) - r["lse"]).abs() <= r["b_lse"]).all())


def test_attention_negative_controls():
    """Each wrong backward leaves the bound on (1, 7, 7, 2) `uniform` f32 - the Dᵢ term dropped (dq, dk), softmax over queries (all
    three), `scale` missing from dk (dk only: dq and dv must still pass)."""
    n, h, w, heads = 1, 7, 7, 2
    scale = PR.f32_scale(SCALE)
    qkv, d_o = PR.attn_inputs("uniform", n, h, w, heads, F32)
    r = PR.attn_fwd_ref(qkv, heads, scale)
    ref, bound = PR.attn_bwd_ref(qkv, r["o"], r["lse"], d_o, heads, scale)
    part = lambda t, a, b: t.reshape(n, h, w, heads, CH)[..., a:b]  # noqa: E731
    for flag, broken, intact in (("drop_D", ["dq", "dk"], ["dv"]), ("softmax_over_queries", ["dq", "dk", "dv"], []),
                                 ("no_scale_dk", ["dk"], ["dq", "dv"])):
        bad, _ = PR.attn_bwd_ref(qkv, r["o"], r["lse"], d_o, heads, scale, **{flag: True})
        out = (bad - ref).abs() > bound
        sl = dict(dq=(0, KD), dk=(KD, 2 * KD), dv=(2 * KD, CH))
        for name in broken:
            assert bool(part(out, *sl[name]).any()), (flag, name)
        for name in intact:
            assert not bool(part(out, *sl[name]).any()), (flag, name)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", DW_CASES, ids=["x".join(map(str, c)) for c in DW_CASES])
def test_depthwise_references_bounds_and_f32_orders(case, family):
    n, h, w, c = case
    for dtype in (F32, BF16):
        x, dz, wt = PR.dw_inputs(family, n, h, w, c, dtype)
        xa = x.to(F64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wa = wt.to(F64).clone().requires_grad_(True)
        za = F.conv2d(xa, wa, None, 1, 1, 1, c)
        (za * dz.to(F64).permute(0, 3, 1, 2)).sum().backward()
        z, bz = PR.dw_fwd_ref(x, wt, dtype)
        dx, bdx, dw, bdw = PR.dw_bwd_ref(x, dz, wt, out_dtype=dtype)
        for got, want in ((z, za.detach().permute(0, 2, 3, 1)), (dx, xa.grad.permute(0, 2, 3, 1)), (dw, wa.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30)
        if family == "uniform" and h * w > 1:
            assert float(bz.max()) <= 2.0 ** -6 * float(z.abs().max()) and float(bdx.max()) <= 2.0 ** -6 * float(dx.abs().max())
            assert float(bdw.max()) <= 2.0 ** -6 * float(dw.abs().max())
        for order in ("natural", "reversed", "partitioned"):
            z32, dx32, dw32 = PR.dw_f32(x, dz, wt, order)
            if dtype == BF16:
                z32, dx32 = z32.to(BF16), dx32.to(BF16)
            assert bool(((z32.to(F64) - z).abs() <= bz).all()) and bool(((dx32.to(F64) - dx).abs() <= bdx).all()), order
            assert bool(((dw32.to(F64) - dw).abs() <= bdw).all()), order
        # accumulate forms: one more term
        dx0, dw0 = torch.ones_like(x), torch.ones_like(wt)
        dxa, _, dwa, _ = PR.dw_bwd_ref(x, dz, wt, dx0, dw0, dtype)
        assert torch.equal(dxa, dx + 1.0) and torch.equal(dwa, dw + 1.0)


def test_depthwise_negative_controls():
    """On (1, 3, 7, 72) `uniform` f32: dx with unflipped taps, dw with (kh, kw) transposed and dw with a padded border pixel counted
    each leave the bound; each control leaves the other output alone."""
    x, dz, wt = PR.dw_inputs("uniform", 1, 3, 7, 72, F32)
    dx, bdx, dw, bdw = PR.dw_bwd_ref(x, dz, wt)
    for flag, which in (("unflipped", "dx"), ("transposed", "dw"), ("count_border", "dw")):
        bx, _, bw, _ = PR.dw_bwd_ref(x, dz, wt, **{flag: True})
        out_x, out_w = bool(((bx - dx).abs() > bdx).any()), bool(((bw - dw).abs() > bdw).any())
        assert (out_x, out_w) == (which == "dx", which == "dw"), flag


def test_new_entries_refuse_bad_arguments_on_the_host():
    """The argument checks run before any launch: no GPU is needed and the buffers keep their bits."""
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    buf = torch.full((1 << 16,), -7.0)
    p = buf.data_ptr()
    o, o2, o3 = p + (1 << 16), p + (2 << 16), p + (3 << 16)
    E, U = L.UPA_EINVAL, L.UPA_EUNSUPPORTED
    s = float(SCALE)
    assert lib.upa_psa_attention_bwd_workspace_bytes(2, 7, 7, 2) == 0 and lib.upa_dwconv2d_bwd_workspace_bytes(64) > 0
    nws = lib.upa_dwconv2d_bwd_workspace_bytes(8)
    fwd = lambda q=p, ld=128, n=1, h=2, w=2, hd=1, kd=32, d=64, out=o, ldo=64, lse=o2, dt=0: lib.upa_psa_attention_train_fwd(  # noqa: E731
        q, ld, n, h, w, hd, kd, d, s, out, ldo, lse, dt, None)
    bwd = lambda q=p, ld=128, oo=o, ldo=64, lse=o2, do=o + 4096, ldd=64, dq=o3, lddq=128, n=1, h=2, w=2, hd=1, kd=32, d=64, dt=0: \
        lib.upa_psa_attention_bwd(q, ld, oo, ldo, lse, do, ldd, dq, lddq, n, h, w, hd, kd, d, s, None, 0, dt, None)  # noqa: E731
    dwf = lambda x=p, n=1, h=2, w=2, c=8, ldx=8, wt=o2, z=o, ldz=8, dt=0: lib.upa_dwconv2d_train_fwd(x, n, h, w, c, ldx, wt, z, ldz, dt, None)  # noqa: E731
    dwb = lambda x=p, dz=p + 4096, n=1, h=2, w=2, c=8, ldx=8, lddz=8, wt=o2, dx=o, lddx=8, dw=o3, ws=o3 + 4096, nw=nws, dt=0: \
        lib.upa_dwconv2d_bwd(x, dz, n, h, w, c, ldx, lddz, wt, dx, lddx, 0, dw, 0, ws, nw, dt, None)  # noqa: E731
    einval = [fwd(q=None), fwd(out=None), fwd(lse=None), fwd(ld=127), fwd(ldo=63), fwd(n=0), fwd(h=0), fwd(out=p + 64),
              bwd(q=None), bwd(oo=None), bwd(lse=None), bwd(do=None), bwd(dq=None), bwd(ld=120), bwd(lddq=127), bwd(ldo=8), bwd(ldd=8),
              bwd(w=0), bwd(dq=p + 64),
              dwf(x=None), dwf(wt=None), dwf(z=None), dwf(c=6, ldx=8), dwf(ldx=4), dwf(ldz=10), dwf(x=p + 4), dwf(n=0), dwf(z=p + 32),
              dwb(dz=None), dwb(dx=None, dw=None), dwb(wt=None), dwb(x=None), dwb(ws=None), dwb(nw=nws - 4), dwb(c=12, ldx=12, lddz=12, lddx=12,
                                                                                                          dt=1),
              dwb(lddz=6), dwb(lddx=9), dwb(dx=p + 4096 + 32)]
    assert einval == [E] * len(einval), einval
    unsupported = [fwd(kd=16), fwd(d=32), fwd(dt=2), bwd(kd=64), bwd(d=128), bwd(dt=3), dwf(dt=2), dwb(dt=7)]
    assert unsupported == [U] * len(unsupported), unsupported
    assert bool((buf == -7.0).all())


def test_trainer_refusals_that_remain():
    """YOLO11 detection (non-legacy Detect head), Dropout(p > 0) and a head_dim other than 64 still have no training path, and YOLO11
    classification trains only with `yolo11=True`."""
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer, DetectionTrainer
    from ultralytics_pro_amd.nn.tasks import ClassificationModel, DetectionModel
    with pytest.raises(UpaError, match="Detect.*no training path"):
        DetectionTrainer(DetectionModel("yolov11n.yaml"))
    m = ClassificationModel("yolov11n-cls.yaml", nc=10)
    m.model[-1].drop.p = 0.1
    with pytest.raises(UpaError, match="Dropout"):
        ClassificationTrainer(m, yolo11=True)
    m = ClassificationModel("yolov11n-cls.yaml", nc=10)
    attn = m.model[9].m[0].attn
    attn.head_dim, attn.key_dim = 32, 16
    with pytest.raises(UpaError, match="head_dim 32"):
        ClassificationTrainer(m, yolo11=True)
    # without the request a YOLO11 model is refused as before, and the message names the switch
    with pytest.raises(UpaError, match="C3k2.*yolo11=True"):
        ClassificationTrainer(ClassificationModel("yolov11n-cls.yaml", nc=10))


def test_flat_layout_puts_the_depthwise_weight_with_the_decayed_weights():
    """oracle.train.param_groups: pe's depthwise conv weight decays, pe's BN weight and bias do not."""
    from oracle import train as otr
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    from ultralytics_pro_amd.parallel import flat_parameter_layout
    m = ClassificationModel("yolov11n-cls.yaml", nc=10)
    groups, meta = flat_parameter_layout(m)
    where = {name: next(i for i, (s, n, _) in enumerate(groups) if s <= off < s + n) for name, off, n, _ in meta}
    decays = [wd for _, _, wd in groups]
    g0, g1, g2 = otr.param_groups(m)
    assert "model.9.m.0.attn.pe.conv.weight" in {k for k, _ in g0} and "model.9.m.0.attn.pe.bn.weight" in {k for k, _ in g1}
    assert decays[where["model.9.m.0.attn.pe.conv.weight"]] and not decays[where["model.9.m.0.attn.pe.bn.weight"]]
    assert not decays[where["model.9.m.0.attn.pe.bn.bias"]]
    assert np.prod(dict(m.named_parameters())["model.9.m.0.attn.pe.conv.weight"].shape) == 128 * 9
