"""Float64 restatements of the training kernels of csrc/psa.hip and csrc/dwconv.hip (upa_psa_attention_train_fwd, upa_psa_attention_bwd,
upa_dwconv2d_train_fwd, upa_dwconv2d_bwd), the per-element error bounds they are held to, and the input families of their tests
(tests/test_psa_train_ref.py on the CPU, tests/test_hip_psa_train.py on the GPU).

Every reference is a sum over explicit indices (einsum / shifted slices), not autograd; tests/test_psa_train_ref.py pins each against
float64 torch.autograd of the reference's own formulation.  Every bound is built from the operands only, u = 2^-24:

    a float32 sum of T terms, in any order, errs by at most (T + c0) u sum|terms|        (c0: the roundings around the sum)

and the attention backward carries it through the chain  s -> P -> dS -> dq / dk:

    s_ij  = scale q_i . k_j          e_s  = (KD + 3) u scale sum|q||k|                     (q * scale rounded, KD fmaf, scale itself)
    P_ij  = exp(s_ij - lse_i)        rho  = e_s + u |s - lse| + EXPF_REL + 2 u   RELATIVE   (an absolute error of the argument is a
                                                                                            relative one of the exponential)
    dp_ij = d_o_i . v_j              e_dp = (HD + 2) u sum|d_o||v|
    D_i   = d_o_i . o_i              e_D  = (HD + 2) u sum|d_o||o|
    dS_ij = P (dp - D)               e_dS = P [ (rho + 3 u) (|dp| + |D|) + e_dp + e_D ],   |dS| <= M_ij = P (|dp| + |D|)
    dv_jc = sum_i P_ij d_o_ic        sum_i P rho |d_o|  +  (N + 2) u sum_i P |d_o|
    dq_ic = scale sum_j dS_ij k_jc   scale [ sum_j e_dS |k|  +  (N + 4) u sum_j M |k| ]
    dk_jc = sum_i dS_ij (scale q_ic) scale [ sum_i e_dS |q|  +  (N + 4) u sum_i M |q| ]

times 1.01 for the higher orders, plus half an output ulp (2^-8 |ref|) where the output is bf16 and 2^-100.  lse and o are INPUTS of the
backward (what the forward stored): the reference takes them as given, so their own error is not part of the backward's bound.
The forward's lse = m + log(sum exp(s - m)): the scores move it by at most max_j e_s, the N-term sum by (N + 2) u relative = absolute
after the logarithm, the exponentials by EXPF_REL, log / the final add (and the log2 -> ln conversion of the matrix-core kernel) by
8 u (|m| + |log l| + 1)."""

import torch

from tests.conv_ref import F64, U24
from tests.yolo11_kernel_ref import EXPF_REL, HD, KD, f32_scale, psa_split

CH = 2 * KD + HD
F32, BF16 = torch.float32, torch.bfloat16
HALF_BF16 = 2.0 ** -8  # bf16 keeps 8 significant bits: round-to-nearest errs by at most half an ulp <= 2^-8 |x|


def _out_ulp(ref, out_dtype):
    return (HALF_BF16 * ref.abs() if out_dtype == BF16 else 0.0) + 2.0 ** -100


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def attn_fwd_ref(qkv, heads, scale):
    """qkv: NHWC (n, h, w, heads * 128).  Returns float64 dict: o (n, h, w, heads * 64), lse (n, heads, N), P, s (n, heads, N, N),
    b_lse (n, heads, N) the bound on lse."""
    n, h, w, _ = qkv.shape
    N = h * w
    scale = f32_scale(scale)
    q, k, v = (t.to(F64) for t in psa_split(qkv, heads))
    s = scale * torch.einsum("bhic,bhjc->bhij", q, k)
    m = s.max(dim=-1).values
    l = torch.exp(s - m.unsqueeze(-1)).sum(-1)
    lse = m + torch.log(l)
    P = torch.exp(s - lse.unsqueeze(-1))
    o = torch.einsum("bhij,bhjc->bhic", P, v)
    e_s = (KD + 3) * U24 * scale * torch.einsum("bhic,bhjc->bhij", q.abs(), k.abs())
    b_lse = 1.01 * (e_s.max(dim=-1).values + (N + 2) * U24 + EXPF_REL + 8 * U24 * (m.abs() + torch.log(l).abs() + 1.0)) + 2.0 ** -100
    return dict(o=o.permute(0, 2, 1, 3).reshape(n, h, w, heads * HD), lse=lse, P=P, s=s, b_lse=b_lse)


def attn_bwd_ref(qkv, o, lse, d_o, heads, scale, out_dtype=F32, drop_D=False, softmax_over_queries=False, no_scale_dk=False):
    """The backward from its inputs AS GIVEN (qkv, the stored o and lse, d_o).  qkv, o, d_o: NHWC; lse: (n, heads, N).  Returns
    (dqkv NHWC float64 in qkv's layout, bound of the same shape).  The three flags build the negative controls."""
    n, h, w, _ = qkv.shape
    N = h * w
    scale = f32_scale(scale)
    q, k, v = (t.to(F64) for t in psa_split(qkv, heads))
    sp = lambda t: t.reshape(n, N, heads, HD).permute(0, 2, 1, 3).to(F64)  # noqa: E731
    oo, do = sp(o), sp(d_o)
    s = scale * torch.einsum("bhic,bhjc->bhij", q, k)
    L = lse.to(F64)
    if softmax_over_queries:
        P = torch.softmax(s, dim=-2)
    else:
        P = torch.exp(s - L.unsqueeze(-1))
    dp = torch.einsum("bhic,bhjc->bhij", do, v)
    D = torch.zeros_like(L) if drop_D else (do * oo).sum(-1)
    dS = P * (dp - D.unsqueeze(-1))
    dv = torch.einsum("bhij,bhic->bhjc", P, do)
    dq = scale * torch.einsum("bhij,bhjc->bhic", dS, k)
    dk = (1.0 if no_scale_dk else scale) * torch.einsum("bhij,bhic->bhjc", dS, q)
    # ---- bounds
    e_s = (KD + 3) * U24 * scale * torch.einsum("bhic,bhjc->bhij", q.abs(), k.abs())
    rho = e_s + U24 * (s - L.unsqueeze(-1)).abs() + EXPF_REL + 2 * U24
    a_dp = torch.einsum("bhic,bhjc->bhij", do.abs(), v.abs())
    a_D = (do.abs() * oo.abs()).sum(-1).unsqueeze(-1)
    e_dp, e_D = (HD + 2) * U24 * a_dp, (HD + 2) * U24 * a_D
    M = P * (dp.abs() + D.abs().unsqueeze(-1))
    e_dS = P * ((rho + 3 * U24) * (dp.abs() + D.abs().unsqueeze(-1)) + e_dp + e_D)
    b_dv = torch.einsum("bhij,bhic->bhjc", P * rho, do.abs()) + (N + 2) * U24 * torch.einsum("bhij,bhic->bhjc", P, do.abs())
    b_dq = scale * (torch.einsum("bhij,bhjc->bhic", e_dS, k.abs()) + (N + 4) * U24 * torch.einsum("bhij,bhjc->bhic", M, k.abs()))
    b_dk = scale * (torch.einsum("bhij,bhic->bhjc", e_dS, q.abs()) + (N + 4) * U24 * torch.einsum("bhij,bhic->bhjc", M, q.abs()))

    def join(a, b, c):  # (n, heads, N, .) x 3 -> NHWC in qkv's layout
        return torch.cat([a, b, c], dim=-1).permute(0, 2, 1, 3).reshape(n, h, w, heads * CH)
    ref = join(dq, dk, dv)
    bound = 1.01 * join(b_dq, b_dk, b_dv) + _out_ulp(ref, out_dtype)
    return ref, bound


def attn_bwd_f32(qkv, o, lse, d_o, heads, scale, order):
    """A float32 emulation of the backward with the summed index (keys for dq, queries for dk / dv, channels for the dots) visited in
    `order`: "natural", "reversed" or "partitioned" (the kernels' split: 16-token partitions of each 64-token block, partition-major)."""
    n, h, w, _ = qkv.shape
    N = h * w

    def perm(L_):
        i = torch.arange(L_)
        if order == "reversed":
            return i.flip(0)
        if order == "partitioned":
            return i[torch.argsort(((i % 64) // 16) * (1 << 20) + i, stable=True)]
        return i
    q, k, v = (t.float() for t in psa_split(qkv, heads))
    sp = lambda t: t.reshape(n, N, heads, HD).permute(0, 2, 1, 3).float()  # noqa: E731
    oo, do = sp(o), sp(d_o)
    sc = torch.tensor(scale, dtype=F32)
    pk, ph, pn = perm(KD), perm(HD), perm(N)
    s = (q * sc)[..., pk] @ k[..., pk].transpose(-1, -2)
    P = torch.exp(s - lse.float().unsqueeze(-1))
    dp = do[..., ph] @ v[..., ph].transpose(-1, -2)
    D = (do[..., ph] * oo[..., ph]).sum(-1, keepdim=True)
    dS = P * (dp - D)
    dv = P[..., pn, :].transpose(-1, -2) @ do[..., pn, :]
    dq = (dS[..., pn] @ k[..., pn, :]) * sc
    dk = dS[..., pn, :].transpose(-1, -2) @ (q * sc)[..., pn, :]
    return torch.cat([dq, dk, dv], dim=-1).permute(0, 2, 1, 3).reshape(n, h, w, heads * CH)


SEAM = 64  # keys / queries per streamed block of csrc/psa.hip


def attn_inputs(family, n, h, w, heads, dtype, key=""):
    """(qkv, d_o) NHWC float32 tensors holding `dtype` values.  uniform: [-1, 1); positive: [0, 1); impulse: zeros with single lit
    queries / keys / pixels at the first and last token and beside the 64-token seam; peaked: q = +-30 / scale along one channel, k one-
    hot, so the scores are +-30 or 0 and P is one-hot to float32."""
    from ultralytics_pro_amd.utils import procedural as Pr
    N = h * w
    tag = f"psatrain:{family}:{n}x{h}x{w}x{heads}:{key}"
    if family in ("uniform", "positive"):
        lo = -1.0 if family == "uniform" else 0.0
        qkv = Pr.uniform(tag + ":qkv", (n, h, w, heads * CH), lo, 1.0)
        d_o = Pr.uniform(tag + ":do", (n, h, w, heads * HD), lo, 1.0)
    elif family == "impulse":
        qkv = torch.zeros(n, N, heads * CH)
        d_o = torch.zeros(n, N, heads * HD)
        lit = sorted({0, N - 1, min(N - 1, SEAM - 1), min(N - 1, SEAM)})
        base = Pr.uniform(tag + ":qkv", (n, N, heads * CH), -1.0, 1.0)
        bd = Pr.uniform(tag + ":do", (n, N, heads * HD), -1.0, 1.0)
        for t in lit:
            qkv[:, t] = base[:, t]
            d_o[:, t] = bd[:, t]
        qkv, d_o = qkv.reshape(n, h, w, -1), d_o.reshape(n, h, w, -1)
    elif family == "peaked":
        qkv = Pr.uniform(tag + ":qkv", (n, N, heads * CH), -1.0, 1.0)
        d_o = Pr.uniform(tag + ":do", (n, h, w, heads * HD), -1.0, 1.0)
        amp = 30.0 / f32_scale(KD ** -0.5)
        for hh in range(heads):
            c0 = hh * CH
            qkv[:, :, c0:c0 + 2 * KD] = 0.0
            for t in range(N):
                ch = t % KD
                qkv[:, t, c0 + ch] = amp if (t // KD) % 2 == 0 else -amp   # query t looks along channel t % 32
                qkv[:, t, c0 + KD + (t * 7 + 3) % KD] = 1.0                 # key t is one-hot
        qkv = qkv.reshape(n, h, w, -1)
    else:
        raise ValueError(family)
    return qkv.to(dtype).float(), d_o.to(dtype).float()


# ---------------------------------------------------------------------------------------------------------------------
# depthwise 3x3, stride 1, pad 1
# ---------------------------------------------------------------------------------------------------------------------
def _shift(x, dy, dx):
    """x (n, h, w, c) -> t with t[:, y, x] = x[:, y + dy, x + dx], zero outside the map."""
    n, h, w, c = x.shape
    t = torch.zeros_like(x)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        t[:, ys:ye, xs:xe] = x[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return t


def dw_fwd_ref(x, wt, out_dtype=F32):
    """x NHWC, wt (C, 1, 3, 3).  z[p, c] = sum_taps w[c, kh, kw] x[p + (kh - 1, kw - 1), c].  Returns (z, bound): 9 terms + 2."""
    x, wt = x.to(F64), wt.to(F64)
    z, S = torch.zeros_like(x), torch.zeros_like(x)
    for kh in range(3):
        for kw in range(3):
            t = _shift(x, kh - 1, kw - 1)
            z += wt[:, 0, kh, kw] * t
            S += wt[:, 0, kh, kw].abs() * t.abs()
    return z, 1.01 * (9 + 2) * U24 * S + _out_ulp(z, out_dtype)


def dw_bwd_ref(x, dz, wt, dx0=None, dw0=None, out_dtype=F32, unflipped=False, transposed=False, count_border=False):
    """dx[p, c] = sum_taps w[c, kh, kw] dz[p - (kh - 1, kw - 1), c] (+ dx0);  dw[c, kh, kw] = sum_p dz[p, c] x[p + (kh - 1, kw - 1), c]
    (+ dw0).  Returns (dx, b_dx, dw, b_dw); dx: 9 (+ 1) terms + 2, dw: n h w (+ 1) terms + 2.  Flags: the negative controls (unflipped
    taps in dx; (kh, kw) transposed in dw; a padded border pixel counted in dw as if the map were edge-replicated)."""
    x, dz, wt = x.to(F64), dz.to(F64), wt.to(F64)
    n, h, w, c = x.shape
    dx, Sx = torch.zeros_like(x), torch.zeros_like(x)
    dw, Sw = torch.zeros(c, 1, 3, 3, dtype=F64), torch.zeros(c, 1, 3, 3, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            sy, sx = ((kh - 1), (kw - 1)) if unflipped else (-(kh - 1), -(kw - 1))
            t = _shift(dz, sy, sx)
            dx += wt[:, 0, kh, kw] * t
            Sx += wt[:, 0, kh, kw].abs() * t.abs()
            xs = _shift(x, kh - 1, kw - 1)
            if count_border:  # the clamp-to-edge read a missing bounds test would make
                yy = (torch.arange(h) + kh - 1).clamp(0, h - 1)
                xx = (torch.arange(w) + kw - 1).clamp(0, w - 1)
                xs = x[:, yy][:, :, xx]
            a, b = (kw, kh) if transposed else (kh, kw)
            dw[:, 0, a, b] = (dz * xs).sum(dim=(0, 1, 2))
            Sw[:, 0, a, b] = (dz.abs() * xs.abs()).sum(dim=(0, 1, 2))
    tx, tw = 9, n * h * w
    if dx0 is not None:
        dx, Sx, tx = dx + dx0.to(F64), Sx + dx0.to(F64).abs(), tx + 1
    if dw0 is not None:
        dw, Sw, tw = dw + dw0.to(F64), Sw + dw0.to(F64).abs(), tw + 1
    return dx, 1.01 * (tx + 2) * U24 * Sx + _out_ulp(dx, out_dtype), dw, 1.01 * (tw + 2) * U24 * Sw + 2.0 ** -100


def dw_f32(x, dz, wt, order):
    """float32 emulation of (z, dx, dw) with the taps / pixels summed in `order` ("natural", "reversed", "partitioned")."""
    x, dz, wt = x.float(), dz.float(), wt.float()
    n, h, w, c = x.shape
    taps = [(a, b) for a in range(3) for b in range(3)]
    if order == "reversed":
        taps = taps[::-1]
    elif order == "partitioned":
        taps = taps[1::2] + taps[0::2]
    z, dx = torch.zeros_like(x), torch.zeros_like(x)
    dw = torch.zeros(c, 1, 3, 3)
    for kh, kw in taps:
        z = z + wt[:, 0, kh, kw] * _shift(x, kh - 1, kw - 1)
        dx = dx + wt[:, 0, kh, kw] * _shift(dz, -(kh - 1), -(kw - 1))
        prod = (dz * _shift(x, kh - 1, kw - 1)).reshape(-1, c)
        if order == "reversed":
            prod = prod.flip(0)
        elif order == "partitioned":
            prod = torch.cat([prod[1::2], prod[0::2]])
        acc = torch.zeros(c)
        for chunk in prod.split(16):
            acc = acc + chunk.sum(0)
        dw[:, 0, kh, kw] = acc
    return z, dx, dw


def dw_inputs(family, n, h, w, c, dtype, key=""):
    """(x, dz NHWC, wt (C, 1, 3, 3) f32) - families as attn_inputs; impulse lights the first and last pixel and, when there is one, an
    interior pixel; peaked: large alternating-sign values (+-30)."""
    from ultralytics_pro_amd.utils import procedural as Pr
    tag = f"dwtrain:{family}:{n}x{h}x{w}x{c}:{key}"
    lo = 0.0 if family == "positive" else -1.0
    x = Pr.uniform(tag + ":x", (n, h, w, c), lo, 1.0)
    dz = Pr.uniform(tag + ":dz", (n, h, w, c), lo, 1.0)
    wt = Pr.uniform(tag + ":w", (c, 1, 3, 3), lo, 1.0)
    if family == "impulse":
        mask = torch.zeros(n, h, w, 1)
        for (yy, xx) in {(0, 0), (h - 1, w - 1), (h // 2, w // 2)}:
            mask[:, yy, xx] = 1.0
        x, dz = x * mask, dz * mask
    elif family == "peaked":
        sign = torch.where(torch.arange(h * w).reshape(1, h, w, 1) % 2 == 0, 1.0, -1.0)
        x, dz = 30.0 * sign * x.abs(), 30.0 * dz
    return x.to(dtype).float(), dz.to(dtype).float(), wt
