"""CPU (-m "not gpu"): the float64 references of tests/mhsa_train_ref.py against float64 torch autograd of the oracle's own MHSA
(oracle/modules.py, imported and not modified) and of F.conv2d, and the C ABI the yolov5-BoT3 training step adds."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mhsa_train_ref as MR

ROOT = Path(__file__).resolve().parents[1]
RTOL = 1e-12


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / max(float(np.abs(ref).max()), 1e-300))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 32), (2, 3, 3, 4, 32), (1, 5, 13, 2, 32), (2, 2, 3, 2, 4), (1, 4, 4, 3, 8), (1, 3, 5, 1, 16),
                                   (1, 2, 2, 2, 64)], ids=lambda s: "n{}_{}x{}_h{}_d{}".format(*s))
def test_forward_and_backward_match_autograd_of_the_oracle_mhsa(shape):
    """out, dq, dk, dv of the numpy statements against torch.autograd through oracle.modules.MHSA in float64.  The module computes
    q / k / v itself, from x through its three 1x1 convs; forward hooks hand the convs' outputs back, so the numpy side gets exactly
    the q, k, v the module used and is compared with the gradients autograd left on those tensors."""
    from oracle.modules import MHSA
    n, h, w, heads, d = shape
    C, L = heads * d, h * w
    m = MHSA(C, heads=heads).double()
    g = torch.Generator().manual_seed(n * 1000 + L * 10 + d)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * C ** -0.5)  # q, k ~ N(0, 1): scores of a few units, so
            # that 1e-12 is a statement about the formulas and not about the cancellation in P (dp - D) of a one-hot softmax
    x = torch.randn(n, C, h, w, generator=g, dtype=torch.float64)
    kept = {}

    def keep(key):
        def hook(mod, inp, out):
            out.retain_grad()
            kept[key] = out
        return hook
    hooks = [conv.register_forward_hook(keep(key)) for key, conv in (("q", m.query), ("k", m.key), ("v", m.value))]
    out = m(x)
    d_o = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(d_o)
    for hk in hooks:
        hk.remove()
    rows = lambda t: t.detach().reshape(n, C, L).permute(0, 2, 1).numpy()  # noqa: E731  NCHW -> (n, L, C)
    q, k, v = rows(kept["q"]), rows(kept["k"]), rows(kept["v"])
    fwd = MR.mhsa_fwd_ref(q, k, v, heads, 1.0)
    assert _rel(fwd["out"], rows(out)) <= RTOL
    # lse is the log of the softmax's denominator: softmax = exp(s - lse)
    s = torch.einsum("bhci,bhcj->bhij", kept["q"].detach().reshape(n, heads, d, L), kept["k"].detach().reshape(n, heads, d, L))
    assert _rel(fwd["lse"], torch.logsumexp(s, -1).numpy()) <= RTOL
    assert _rel(fwd["P"], s.softmax(-1).numpy()) <= RTOL
    (dq, dk, dv), bounds = MR.mhsa_bwd_ref(q, k, v, fwd["lse"], rows(d_o), heads, 1.0)
    assert _rel(dq, rows(kept["q"].grad)) <= RTOL
    assert _rel(dk, rows(kept["k"].grad)) <= RTOL
    assert _rel(dv, rows(kept["v"].grad)) <= RTOL
    assert all(np.isfinite(b).all() and (b > 0).all() for b in bounds)
    if L == 1:  # one token: P = 1, so the scores get no gradient and dv = d_o
        assert np.all(dq == 0) and np.all(dk == 0) and np.array_equal(dv, rows(d_o))


def test_scaled_form_and_residual_match_autograd():
    """scale != 1 (nn.MultiheadAttention's use of the same kernel) and the fused residual: float64 autograd of the plain formula."""
    n, L, heads, d = 2, 7, 2, 8
    g = torch.Generator().manual_seed(5)
    q, k, v, res, d_o = (torch.randn(n, L, heads * d, generator=g, dtype=torch.float64) for _ in range(5))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    scale = float(np.float32(d ** -0.5))
    sp = lambda t: t.reshape(n, L, heads, d).permute(0, 2, 1, 3)  # noqa: E731
    P = (scale * sp(q) @ sp(k).transpose(-1, -2)).softmax(-1)
    out = (P @ sp(v)).permute(0, 2, 1, 3).reshape(n, L, heads * d) + res
    out.backward(d_o)
    fwd = MR.mhsa_fwd_ref(q.detach().numpy(), k.detach().numpy(), v.detach().numpy(), heads, scale, residual=res.numpy())
    assert _rel(fwd["out"], out.detach().numpy()) <= RTOL
    (dq, dk, dv), _ = MR.mhsa_bwd_ref(q.detach().numpy(), k.detach().numpy(), v.detach().numpy(), fwd["lse"], d_o.numpy(), heads, scale)
    assert _rel(dq, q.grad.numpy()) <= RTOL and _rel(dk, k.grad.numpy()) <= RTOL and _rel(dv, v.grad.numpy()) <= RTOL


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_the_120_magnitude_case_is_finite_in_float64_and_would_overflow_float32_without_the_running_max(bf16):
    q, k, v, d_o, _ = MR.mhsa_inputs("big", 1, 65, 2, 32, bf16, magnitude=120.0)
    fwd = MR.mhsa_fwd_ref(q, k, v, 2)
    assert 100.0 <= float(np.abs(fwd["s"]).max()) <= 140.0
    assert np.isfinite(fwd["lse"]).all() and np.isfinite(fwd["out"]).all()
    (dq, dk, dv), bounds = MR.mhsa_bwd_ref(q, k, v, fwd["lse"], d_o, 2)
    assert all(np.isfinite(t).all() for t in (dq, dk, dv) + bounds)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(fwd["s"].astype(np.float32))).all()  # exp(100) is past float32


@pytest.mark.parametrize("shape", [(2, 16, 16, 16), (1, 20, 12, 24), (2, 6, 6, 16), (1, 9, 7, 8)], ids=lambda s: "n{}_{}x{}_c{}".format(*s))
def test_k6_weight_gradient_matches_conv2d_autograd(shape):
    n, h, w, cout = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, 3, 6, 6, generator=g, dtype=torch.float64, requires_grad=True)
    z = F.conv2d(x, wt, stride=2, padding=2)
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    z.backward(dz)
    got = MR.wgrad_k6_ref(x.permute(0, 2, 3, 1).numpy(), dz.permute(0, 2, 3, 1).numpy())
    assert _rel(got, wt.grad.numpy()) <= RTOL
    ref2 = torch.nn.grad.conv2d_weight(x, (cout, 3, 6, 6), dz, stride=2, padding=2)
    assert _rel(got, ref2.numpy()) <= RTOL


def test_bf16_round_is_torchs():
    a = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 37.0
    assert np.array_equal(MR.bf16_round(a.numpy()), a.to(torch.bfloat16).float().numpy())


def test_the_training_abi_of_bot3_is_exported_and_bound():
    """The built library exports the MHSA training entries, _lib.py binds them with the header's argument counts, and the stem's weight
    gradient has a workspace (other 6x6 shapes have none)."""
    import ctypes
    from ultralytics_pro_amd import _lib as L
    if not L.LIB_PATH.is_file():
        import __graft_entry__ as g
        g.build()
    handle = ctypes.CDLL(str(L.LIB_PATH))
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "upa.h").read_text(), flags=re.S)
    for name in ("upa_mhsa_train_fwd", "upa_mhsa_bwd", "upa_mhsa_bwd_workspace_bytes"):
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in L.PROTOTYPES, f"{name} has no ctypes prototype"
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert decl, f"{name} is not declared in include/upa.h"
        assert len(L.PROTOTYPES[name][1]) == len(decl.group(1).split(",")), f"{name}: prototype and declaration disagree"
    lib = L.lib()
    assert lib.upa_conv2d_wgrad_workspace_bytes(3, 16, 6) > 0
    assert lib.upa_conv2d_wgrad_workspace_bytes(3, 64, 6) == 4 * lib.upa_conv2d_wgrad_workspace_bytes(3, 16, 6)
    assert lib.upa_conv2d_wgrad_workspace_bytes(16, 16, 6) == 0
    assert lib.upa_mhsa_bwd_workspace_bytes(2, 400, 4) == 2 * 400 * 4 * 4
    # refusals are host logic: no GPU is needed to see them (nothing is launched)
    one = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(one)
    assert lib.upa_mhsa_bwd(p, p + 256, p + 512, 96, p + 1024, p + 2048, 32, p + 3072, p + 3200, p + 3328, 96, 1, 1, 1, 24, 1.0, p + 3500, 64,
                            L.UPA_F32, None) == L.UPA_EUNSUPPORTED                                  # head width 24
    assert lib.upa_mhsa_bwd(p, p + 256, p + 512, 96, p + 1024, p + 2048, 32, p, p + 3200, p + 3328, 96, 1, 1, 1, 32, 1.0, p + 3500, 64,
                            L.UPA_F32, None) == L.UPA_EINVAL                                        # dq is q
    assert lib.upa_mhsa_train_fwd(p, p + 256, p + 512, 96, 1, 1, 1, 24, 1.0, None, 0, p + 2048, 32, p + 3072, L.UPA_F32,
                                  None) == L.UPA_EUNSUPPORTED


def test_trainer_names_the_layer_it_refuses_and_keeps_convt_text():
    """Host-side construction rules of the new trainer ops: the stem form only where no data gradient is asked for, and the unchanged
    refusal text for every other kernel size."""
    import torch.nn as nn
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine import trainer as T
    from ultralytics_pro_amd.nn.modules import block as B

    class Ctx:  # the constructor paths under test raise before they touch the device
        device, dtype, code, es, E = torch.device("cpu"), torch.float32, 0, 4, 4
    with pytest.raises(UpaError, match=r"training supports k in \(1,3\), stride in \(1,2\) \(stem: k=6 s=2\)"):
        T.ConvT(Ctx, nn.Conv2d(3, 16, 6, 2, 2, bias=False), nn.BatchNorm2d(16), 1, "stem")
    with pytest.raises(UpaError, match=r"training supports k in \(1,3\)"):
        T.ConvT(Ctx, nn.Conv2d(3, 16, 5, 2, 2, bias=False), nn.BatchNorm2d(16), 1, "stem", no_dgrad=True)
    with pytest.raises(UpaError, match=r"model\.10\.m\.0\.cv2\.0.*head widths"):
        T.MHSAT(Ctx, B.MHSA(96, heads=4), "model.10.m.0.cv2.0")
