"""Float64 CPU restatements of `upa_classify_pool` and `upa_softmax_topk` (csrc/classify.hip) and the per-element error bounds their
kernels are held to.  Plain torch on the CPU, built on tests/conv_ref.py; nothing here imports the HIP package's kernels.
tests/test_classify_oracle.py pins these functions (a loop implementation, an f32 emulation in two summation orders, two negative
controls); tests/test_hip_classify.py compares the kernels with them."""

import torch

from tests import conv_ref as CR

F64 = torch.float64
U24 = CR.U24


def pool_ref(x, w, bias, act):
    """x: (n, cin, h, w) NCHW, w: (cout, cin) or OIHW 1x1, bias: (cout) - values their storage type represents exactly.  Returns float64
    (ref (n, cout), bound (n, cout)):
      ref    = (1 / HW) * sum_p act(v_p),  v_p = bias + sum_k x[p, k] W[c, k]            (`conv_ref` with k = 1)
      bound  = (1 / HW) * sum_p [ L 1.01 (K + 1) 2^-24 S_p + (|v_p| + 6) 2^-24 |act(v_p)| ]   conv_bound's accumulation and activation
                                                                                             terms per pixel, f32 result (L = 1.1 for
                                                                                             SiLU; the activation term for SiLU only)
             + 1.01 (HW + 1) 2^-24 (1 / HW) sum_p |act(v_p)|                             an f32 sum of HW values in any order + the scale
             + 2^-23 |ref|                                                               the final store
    with K = cin.  No element is excluded."""
    w4 = w.reshape(w.shape[0], w.shape[1], 1, 1)
    v, S, a = CR.conv_ref(x, w4, bias, None, 1, 1, 0, act)
    n, cout, h, wd = a.shape
    hw = h * wd
    K = x.shape[1]
    ref = a.sum((2, 3)) / hw
    lip = 1.1 if act == CR.ACT_SILU else 1.0
    per = lip * 1.01 * (K + 1) * U24 * S
    if act == CR.ACT_SILU:
        per = per + (v.abs() + 6.0) * U24 * a.abs()
    bound = per.sum((2, 3)) / hw + 1.01 * (hw + 1) * U24 * a.abs().sum((2, 3)) / hw + 2.0 ** -23 * ref.abs()
    return ref, bound


def pool_loop(x, w, bias, act):
    """`pool_ref`'s value by explicit loops over image, channel, pixel and input channel (float64; tiny shapes only)."""
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    out = torch.zeros(n, cout, dtype=F64)
    for i in range(n):
        for c in range(cout):
            tot = 0.0
            for py in range(h):
                for px in range(wd):
                    v = float(bias[c])
                    for k in range(cin):
                        v += float(x[i, k, py, px]) * float(w[c, k])
                    tot += float(CR.act_ref(torch.tensor(v, dtype=F64), act))
            out[i, c] = tot / (h * wd)
    return out


def pool_f32_emulation(x, w, bias, act, order="forward", pad_rows=0, pad_mode=None):
    """The kernel's arithmetic in float32 on the CPU: per pixel an f32 dot product + bias, the activation in f32, an f32 sum over the
    pixels in `order` ('forward' | 'reverse' | 'pairwise') and one f32 divide.  The two negative controls model the padded-row bugs:
    pad_mode 'act_bias' adds `pad_rows` rows of value act(bias) to the sum, 'count' divides by HW + pad_rows."""
    n, cin, h, wd = x.shape
    hw = h * wd
    xf = x.float().permute(0, 2, 3, 1).reshape(n, hw, cin)
    v = torch.einsum("npk,ck->npc", xf, w.float().reshape(w.shape[0], cin)) + bias.float()
    a = v / (1.0 + torch.exp(-v)) if act == CR.ACT_SILU else v
    rows = [a[:, p] for p in range(hw)]
    if pad_mode == "act_bias":
        b = bias.float()
        rows += [(b / (1.0 + torch.exp(-b)) if act == CR.ACT_SILU else b).expand(n, -1)] * pad_rows
    if order == "reverse":
        rows = rows[::-1]
    if order == "pairwise":
        while len(rows) > 1:
            rows = [rows[i] + rows[i + 1] if i + 1 < len(rows) else rows[i] for i in range(0, len(rows), 2)]
        tot = rows[0]
    else:
        tot = rows[0].clone()
        for r_ in rows[1:]:
            tot = tot + r_
    return tot / float(hw + (pad_rows if pad_mode == "count" else 0))


def softmax_ref(z):
    """z: (rows, nc) float32 logits (-inf allowed, no NaN, a finite row maximum).  Returns float64 (probs, bound, row-sum tolerance):
      |p_i - ref_i| <= 1.01 (2 D + nc + 8) 2^-24 ref_i + 2^-126,   D = max_j |z_j - max z| over the row's finite logits
        (z - max is one rounding of a number up to D: the exponential's argument errs by D 2^-24 in numerator and denominator; the f32 sum of
        nc terms, expf, the divide and the store are the nc + 8 units; terms below 2^-126 may flush to zero)
      |sum_i p_i - 1| <= (nc + 8) 2^-24."""
    z64 = z.to(F64)
    m = z64.max(1, keepdim=True).values
    d = z64 - m
    fin = torch.isfinite(d)
    D = torch.where(fin, d.abs(), torch.zeros_like(d)).max(1, keepdim=True).values
    e = torch.exp(d)
    ref = e / e.sum(1, keepdim=True)
    nc = z.shape[1]
    bound = 1.01 * (2 * D + nc + 8) * U24 * ref + 2.0 ** -126
    return ref, bound, (nc + 8) * U24


def topk_ref(z, k):
    """Indices of the k largest logits per row, descending, ties to the lower index: a stable descending sort of the input."""
    return torch.sort(z, dim=1, descending=True, stable=True).indices[:, :k].to(torch.int32)
