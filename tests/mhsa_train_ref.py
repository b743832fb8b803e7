"""Float64 numpy statements of the training kernels this model family adds (csrc/attention.hip: upa_mhsa_train_fwd, upa_mhsa_bwd;
csrc/train.hip: the 6x6 stride-2 pad-2 stem weight gradient), the per-element error bounds the attention kernels are held to, and the
input families of their tests (tests/test_mhsa_train_ref.py on the CPU, tests/test_hip_bot3_train.py on the GPU).

Every reference is a sum over explicit indices (einsum / shifted slices), not autograd; tests/test_mhsa_train_ref.py pins each against
float64 torch.autograd of the oracle's own MHSA.  Rows are (n, L, heads * d) arrays: token-major, a head's d channels contiguous - the
q / k / v channel slices of the [q | k | v] buffer the three 1x1 convs write.

The bounds follow tests/psa_train_ref.py (the same u = 2^-24, EXPF_REL and 1.01 for the higher orders; a float32 sum of T terms in any
order errs by at most (T + c0) u sum|terms|), with one difference: D is not d_o . o but the kernel's own sum over the keys,

    s_ij  = scale q_i . k_j          e_s  = (d + 3) u scale sum|q||k|
    P_ij  = exp(s_ij - lse_i)        rho  = e_s + u |s - lse| + EXPF_REL + 2 u                RELATIVE
    dp_ij = d_o_i . v_j              e_dp = (d + 2) u sum|d_o||v|
    D_i   = sum_j P_ij dp_ij         e_D  = sum_j P (rho |dp| + e_dp)  +  (L + 2) u sum_j P |dp|
    dS_ij = P (dp - D)               e_dS = P [ (rho + 3 u) (|dp| + |D|) + e_dp + e_D ],   |dS| <= M_ij = P (|dp| + |D|)
    dv_jc = sum_i P_ij d_o_ic        sum_i P rho |d_o|  +  (L + 2) u sum_i P |d_o|
    dq_ic = scale sum_j dS_ij k_jc   scale [ sum_j e_dS |k|  +  (L + 4) u sum_j M |k| ]
    dk_jc = sum_i dS_ij (scale q_ic) scale [ sum_i e_dS |q|  +  (L + 4) u sum_i M |q| ]

plus half an output ulp (2^-8 |ref|) where the output is bf16, and 2^-100.  lse is an INPUT of the backward (what the forward stored):
the reference takes it as given.  The forward's lse is bounded as psa_train_ref.attn_fwd_ref bounds it."""

import numpy as np

from tests.psa_train_ref import HALF_BF16  # the gate constants of upa_psa_attention_bwd's test, reused
from tests.yolo11_kernel_ref import EXPF_REL, U24

MHSA_DIMS = (4, 8, 16, 32, 64)


def split_heads(rows, heads):
    """(n, L, heads * d) -> (n, heads, L, d) float64"""
    n, L, C = rows.shape
    return np.asarray(rows, dtype=np.float64).reshape(n, L, heads, C // heads).transpose(0, 2, 1, 3)


def join_heads(t):
    """(n, heads, L, d) -> (n, L, heads * d)"""
    n, heads, L, d = t.shape
    return t.transpose(0, 2, 1, 3).reshape(n, L, heads * d)


def f32(x):
    return float(np.float32(x))


def mhsa_fwd_ref(q, k, v, heads, scale=1.0, residual=None):
    """out (n, L, C) (+ residual), lse (n, heads, L), P, s (n, heads, L, L), b_lse: all float64."""
    scale = f32(scale)
    qh, kh, vh = (split_heads(t, heads) for t in (q, k, v))
    d = qh.shape[-1]
    L = qh.shape[2]
    s = scale * np.einsum("bhic,bhjc->bhij", qh, kh)
    m = s.max(-1)
    l = np.exp(s - m[..., None]).sum(-1)
    lse = m + np.log(l)
    P = np.exp(s - lse[..., None])
    out = join_heads(np.einsum("bhij,bhjc->bhic", P, vh))
    if residual is not None:
        out = out + np.asarray(residual, dtype=np.float64)
    e_s = (d + 3) * U24 * scale * np.einsum("bhic,bhjc->bhij", np.abs(qh), np.abs(kh))
    b_lse = 1.01 * (e_s.max(-1) + (L + 2) * U24 + EXPF_REL + 8 * U24 * (np.abs(m) + np.abs(np.log(l)) + 1.0)) + 2.0 ** -100
    return dict(out=out, lse=lse, P=P, s=s, b_lse=b_lse)


def mhsa_bwd_ref(q, k, v, lse, d_o, heads, scale=1.0, bf16_out=False):
    """The backward from its inputs as given.  Returns (dq, dk, dv) and their bounds, each (n, L, C) float64."""
    scale = f32(scale)
    qh, kh, vh, do = (split_heads(t, heads) for t in (q, k, v, d_o))
    d, L = qh.shape[-1], qh.shape[2]
    Lq = np.asarray(lse, dtype=np.float64)[..., None]
    s = scale * np.einsum("bhic,bhjc->bhij", qh, kh)
    P = np.exp(s - Lq)
    dp = np.einsum("bhic,bhjc->bhij", do, vh)
    D = (P * dp).sum(-1, keepdims=True)
    dS = P * (dp - D)
    dv = np.einsum("bhij,bhic->bhjc", P, do)
    dq = scale * np.einsum("bhij,bhjc->bhic", dS, kh)
    dk = scale * np.einsum("bhij,bhic->bhjc", dS, qh)
    # ---- bounds
    e_s = (d + 3) * U24 * scale * np.einsum("bhic,bhjc->bhij", np.abs(qh), np.abs(kh))
    rho = e_s + U24 * np.abs(s - Lq) + EXPF_REL + 2 * U24
    e_dp = (d + 2) * U24 * np.einsum("bhic,bhjc->bhij", np.abs(do), np.abs(vh))
    e_D = (P * (rho * np.abs(dp) + e_dp)).sum(-1, keepdims=True) + (L + 2) * U24 * (P * np.abs(dp)).sum(-1, keepdims=True)
    M = P * (np.abs(dp) + np.abs(D))
    e_dS = P * ((rho + 3 * U24) * (np.abs(dp) + np.abs(D)) + e_dp + e_D)
    b_dv = np.einsum("bhij,bhic->bhjc", P * rho, np.abs(do)) + (L + 2) * U24 * np.einsum("bhij,bhic->bhjc", P, np.abs(do))
    b_dq = scale * (np.einsum("bhij,bhjc->bhic", e_dS, np.abs(kh)) + (L + 4) * U24 * np.einsum("bhij,bhjc->bhic", M, np.abs(kh)))
    b_dk = scale * (np.einsum("bhij,bhic->bhjc", e_dS, np.abs(qh)) + (L + 4) * U24 * np.einsum("bhij,bhic->bhjc", M, np.abs(qh)))
    refs = tuple(join_heads(t) for t in (dq, dk, dv))
    bounds = tuple(1.01 * join_heads(b) + (HALF_BF16 * np.abs(r) if bf16_out else 0.0) + 2.0 ** -100
                   for b, r in zip((b_dq, b_dk, b_dv), refs))
    return refs, bounds


def bf16_round(a):
    """float -> the nearest bfloat16 value (ties to even), as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(a.shape)


def mhsa_inputs(tag, n, L, heads, d, bf16, magnitude=None):
    """(q, k, v, d_o, residual) float32 (n, L, heads * d) arrays holding values of the storage type.  uniform [-1, 1); with `magnitude` q
    and k are scaled so that the largest |q . k| over the case is `magnitude` (then rounded to the storage type: a few per cent off)."""
    from ultralytics_pro_amd.utils import procedural as P
    C = heads * d
    t = {name: P.uniform(f"mhsatrain:{tag}:{name}:{n}x{L}x{heads}x{d}", (n, L, C), -1.0, 1.0).numpy().astype(np.float32)
         for name in ("q", "k", "v", "do", "res")}
    if magnitude is not None:
        s = np.einsum("bhic,bhjc->bhij", split_heads(t["q"], heads), split_heads(t["k"], heads))
        f = np.float32(np.sqrt(magnitude / np.abs(s).max()))
        t["q"], t["k"] = t["q"] * f, t["k"] * f
    if bf16:
        t = {key: bf16_round(val) for key, val in t.items()}
    return t["q"], t["k"], t["v"], t["do"], t["res"]


# ---------------------------------------------------------------------------------------------------------------------
# the 6x6 stride-2 pad-2 weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_k6_ref(x, dz):
    """x (n, h, w, 3), dz (n, oh, ow, cout), oh = (h + 4 - 6) // 2 + 1: dW (cout, 3, 6, 6) float64,
    dW[co, ci, kh, kw] = sum_{n, oy, ox} dz[n, oy, ox, co] x[n, 2 oy + kh - 2, 2 ox + kw - 2, ci]."""
    x, dz = np.asarray(x, dtype=np.float64), np.asarray(dz, dtype=np.float64)
    n, h, w, cin = x.shape
    _, oh, ow, cout = dz.shape
    assert (oh, ow) == ((h + 4 - 6) // 2 + 1, (w + 4 - 6) // 2 + 1)
    xp = np.zeros((n, 2 * oh + 4, 2 * ow + 4, cin))
    xp[:, 2:2 + h, 2:2 + w] = x
    dw = np.zeros((cout, cin, 6, 6))
    for kh in range(6):
        for kw in range(6):
            win = xp[:, kh:kh + 2 * oh:2, kw:kw + 2 * ow:2]
            dw[:, :, kh, kw] = np.einsum("nyxo,nyxi->oi", dz, win)
    return dw
