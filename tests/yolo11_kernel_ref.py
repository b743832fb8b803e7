"""Float64 CPU restatements of `upa_dwconv2d` (csrc/dwconv.hip), `upa_psa_attention` (csrc/psa.hip) and `upa_conv_transpose2x2`
(csrc/segment.hip), the per-element error bounds their kernels are held to and the input families of the tests.

Plain torch on the CPU; nothing here imports the HIP package's kernels or the oracle.  tests/test_yolo11_kernel_ref.py pins these
functions (against nested loops, hand-worked values and float32 emulations of the kernels' arithmetic order, mutated and not);
tests/test_hip_yolo11_kernels.py compares the kernels with them."""

import math

import torch
import torch.nn.functional as F

from tests.conv_ref import ACT_NONE, ACT_SILU, F64, U24, act_ref, conv_bound, impulse_positions, stored

KD, HD = 32, 64        # key_dim / head_dim of every YOLO11 scale: per head the qkv channels are [q 32 | k 32 | v 64]
CH = 2 * KD + HD
PSA_KB, PSA_KP = 64, 4  # csrc/psa.hip: keys per LDS block, key partitions (waves) of the scalar kernel
SCALE = KD ** -0.5      # v10_Attention.scale

# Relative error of the exponentials psa.hip calls, over the arguments an online softmax forms (score - running maximum <= 0).
# Neither the guides nor the ROCm documentation on hand state it, so the functions themselves (not the kernels under test) were
# measured on an MI355X against float64 with tools/experiments/exp_error.hip (2^28 evenly spaced arguments and 2^22 mantissas in
# each of the 40 binades of magnitude 2^-40 .. 1; ROCm 7.2, -O3 -ffp-contract=off as the library is built):
#   expf                            on [-130, 0]: max relative error 1.4108 * 2^-24; expf(0) = expf(-0) = 1, expf(-inf) = 0 exactly
#   __builtin_amdgcn_exp2f (v_exp)  on [-190, 0]: max relative error 1.4234 * 2^-24; 1 / 1 / 0 likewise; results below 2^-126 are
#                                   flushed (absolute error 2^-126, which the bounds' 2^-100 absorbs: see psa_bound)
# The ranges cover what the tests reach (logit spread <= 125, * log2(e) = 180 for exp2).  A sample is no proof: the constants carry
# a factor of two of margin.
EXPF_REL = 3.0 * U24   # >= 2 * 1.4108 * 2^-24
EXP2_REL = 3.0 * U24   # >= 2 * 1.4234 * 2^-24


def f32_scale(scale):
    """The float the C ABI receives for `scale`."""
    return float(torch.tensor(scale, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# upa_dwconv2d
# ---------------------------------------------------------------------------------------------------------------------
def dw_out_hw(h, w, stride):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def dw_ref(x, w9c, bias, stride, act):
    """Depthwise 3x3, pad 1.  x: NCHW, w9c: (9, c) in the kernel's layout (tap = ky * 3 + kx major), bias: (c).  Returns float64 NCHW
      v    bias + sum_tap w[tap, c] * x[c, oy * stride - 1 + ky, ox * stride - 1 + kx]  (taps outside the map contribute nothing),
      S    the same on absolute operands,
      ref  act(v);
    the kernel is held to conv_bound(v, S, ref, 9, act, out_dtype)."""
    n, c, h, w = x.shape
    assert w9c.shape == (9, c) and bias.shape == (c,) and stride in (1, 2)
    oh, ow = dw_out_hw(h, w, stride)
    xp = F.pad(x.to(F64), (1, 1, 1, 1))
    w64, b64 = w9c.to(F64), bias.to(F64).view(1, c, 1, 1)
    v = b64.expand(n, c, oh, ow).clone()
    S = b64.abs().expand(n, c, oh, ow).clone()
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, :, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride]
            wt = w64[ky * 3 + kx].view(1, c, 1, 1)
            v += sl * wt
            S += sl.abs() * wt.abs()
    return v, S, act_ref(v, act)


def dw_bound(v, S, ref, act, out_dtype):
    return conv_bound(v, S, ref, 9, act, out_dtype)


# ---------------------------------------------------------------------------------------------------------------------
# upa_conv_transpose2x2
# ---------------------------------------------------------------------------------------------------------------------
def convt_ref(x, w, bias):
    """nn.ConvTranspose2d(k 2, s 2, p 0): out[n, co, 2y + i, 2x + j] = bias[co] + sum_ci x[n, ci, y, x] * W[ci, co, i, j].
    x: NCHW, w: (cin, cout, 2, 2) holding what the packed weight holds (for bf16: already rounded to nearest even, as
    `upa_pack_conv_transpose2x2_weight` rounds), bias: (cout).  Returns float64 (v, S, ref = v) as (n, cout, 2h, 2w); the kernel is
    held to conv_bound(v, S, ref, cin, ACT_NONE, out_dtype)."""
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    assert w.shape == (cin, cout, 2, 2) and bias.shape == (cout,)
    b64 = bias.to(F64).view(1, cout, 1, 1)
    v = torch.einsum("ncyx,cdij->ndyixj", x.to(F64), w.to(F64)).reshape(n, cout, 2 * h, 2 * wd) + b64
    S = torch.einsum("ncyx,cdij->ndyixj", x.to(F64).abs(), w.to(F64).abs()).reshape(n, cout, 2 * h, 2 * wd) + b64.abs()
    return v, S, v.clone()


def convt_bound(v, S, ref, cin, out_dtype):
    return conv_bound(v, S, ref, cin, ACT_NONE, out_dtype)


def convt_pack_ref(w, dtype):
    """The packed weight as documented in csrc/segment.hip: (4 * cout, kp) with row q = tap * cout + co (tap = 2 i + j), kp = cin rounded
    up to the MFMA depth (bf16 32, f32 4), zero filled, rounded to nearest even for bf16.  Returns float32 (the stored values)."""
    cin, cout = w.shape[:2]
    kb = 32 if dtype == torch.bfloat16 else 4
    kp = -(-cin // kb) * kb
    out = torch.zeros(4 * cout, kp)
    out[:, :cin] = w.float().permute(2, 3, 1, 0).reshape(4 * cout, cin)
    return stored(out, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# upa_psa_attention
# ---------------------------------------------------------------------------------------------------------------------
def psa_split(qkv, heads):
    """NHWC (n, h, w, heads * 128) -> q (n, heads, N, 32), k (n, heads, N, 32), v (n, heads, N, 64)."""
    n, h, w, c = qkv.shape
    assert c == heads * CH
    x = qkv.reshape(n, h * w, heads, CH).permute(0, 2, 1, 3)
    return x[..., :KD], x[..., KD:2 * KD], x[..., 2 * KD:]


def psa_ref(qkv, h, w, heads, scale, pe_w9c, pe_b):
    """qkv: NHWC (n, h, w, heads * 128); pe_w9c: (9, heads * 64) tap-major; pe_b: (heads * 64); scale: the float the kernel receives.
    Per (image, head), with N = h * w tokens in row-major pixel order:
        logits[p, q] = scale * sum_i q[p, i] k[q, i],  attn = softmax over q,
        out[p, j] = sum_q attn[p, q] v[q, j] + pe(v)[p, j],   pe = depthwise 3x3 (pad 1, no activation) of v as an h x w image.
    Returns a dict of float64 tensors; the NHWC ones are (n, h, w, heads * 64):
        out     the result                                    A    sum_q attn[p, q] |v[q, j]|   (NHWC)
        Sqk     scale * max_q sum_i |q[p, i] k[q, i]|, broadcast over the head's 64 channels  (NHWC)
        peS     |pe_b| + sum_tap |w| |v|  (NHWC)              logits, attn   (n, heads, N, N)"""
    n = qkv.shape[0]
    N = h * w
    scale = f32_scale(scale)
    q, k, v = (t.to(F64) for t in psa_split(qkv, heads))
    logits = scale * (q @ k.transpose(-1, -2))
    attn = torch.softmax(logits, dim=-1)

    def nhwc(t):  # (n, heads, N, 64) -> (n, h, w, heads * 64)
        return t.permute(0, 2, 1, 3).reshape(n, h, w, heads * HD)
    o, A = nhwc(attn @ v), nhwc(attn @ v.abs())
    sqk = scale * (q.abs() @ k.abs().transpose(-1, -2)).max(dim=-1).values           # (n, heads, N)
    Sqk = nhwc(sqk.unsqueeze(-1).expand(n, heads, N, HD))
    vimg = nhwc(v).permute(0, 3, 1, 2)                                               # (n, heads * 64, h, w)
    pe, peS, _ = dw_ref(vimg, pe_w9c, pe_b, 1, ACT_NONE)
    pe, peS = pe.permute(0, 2, 3, 1), peS.permute(0, 2, 3, 1)
    return dict(out=o + pe, A=A, Sqk=Sqk, peS=peS.contiguous(), logits=logits, attn=attn)


def psa_part_keys(N):
    """Keys the fullest partition (partition 0) of the scalar kernel walks: 16 of every full 64-key block and up to 16 of the last."""
    return 16 * (N // PSA_KB) + min(16, N % PSA_KB)


def psa_bound(kind, r, N, out_dtype):
    """Per-element bound on |kernel - r["out"]| for kind = "scalar" (psa_attn_kernel<float | bf16, 32, 64>) or "mfma"
    (psa_attn_mfma_kernel), derived from what the kernels do (u = 2^-24; every first-order term carries 1.01 for the higher orders):

        2 E_w A  +  c_acc u A  +  [mfma: 2^-8 A]  +  10 u peS  +  u_out |ref|  +  2^-100

    Both kernels return sum_q w_q v_q / sum_q w_q with computed weights w_q = exp(s_q - M) (1 + eta_q); the common factor exp(-M)
    cancels whatever M is.  With |eta_q| <= E_w, numerator and denominator each move by at most E_w (times A, times 1), so the
    quotient moves by at most 2 E_w A.  E_w collects, per key:
      logit        scalar: q * scale rounded, then 32 fmaf: 33 u * sum|q k| scale <= 33 u Sqk.  mfma: 32 exact bf16 products summed in
                   f32 by one MFMA (any order: 32 u), the product with c_log2 = scale * log2(e), itself a rounded float (u each on a
                   value <= Sqk): 35 u Sqk.  An absolute logit error is a relative weight error.
      arguments    the subtractions s - m and m - m' feeding the exponentials round by u |argument|; along one key's chain (its own
                   exponential, every later rise of the running maximum, the merge) the arguments are all <= 0 and add up to at most
                   the logit spread <= 2 Sqk: 2 u Sqk in all (in log2 units for the mfma kernel, which is the same relative weight
                   error).
      exponentials each call errs by EXPF_REL / EXP2_REL (see above).  A rescale whose maximum did not rise is exp(0) = 1 exactly and
                   costs nothing, so the count is the key's own call plus the rises after it.  scalar: the maximum can rise at every
                   key of the partition, P = psa_part_keys(N) in the fullest, plus the merge: (P + 1) calls.  mfma: one rescale per
                   64-key block and no merge: ceil(N / 64) calls.
    Accumulation, c_acc (every count is of f32 roundings a term passes through):
      scalar       numerator: o * alpha and the fmaf per key, 2 P; merge o * a0, three fmaf, o * inv: 5.  denominator: l * alpha + p
                   per key (the library is built with -ffp-contract=off: two roundings), 2 P; merge l * a0, three (multiply, add): 4
                   (counted as 1 + 3: the products are the terms' own); 1 / l: 1.  c_acc = 4 P + 11.
      mfma         numerator: per block o * alpha and two MFMAs of 32 products each (any order), 65 per block; o * inv: 1.  denominator:
                   16 adds into ps, l * alpha + ps, per block 18; two cross-lane adds and 1 / l: 3.  c_acc = 83 ceil(N / 64) + 4.
    mfma only: each probability is rounded to bf16 (round to nearest even: pack_bf16x2 is v_cvt_pk_bf16_f32; eight significant bits, so
    half an ulp is up to 2^-8 relative) before the P . V product while the denominator sums the unrounded values, so the numerator
    alone moves by 2^-8 A.
    pe: bias and nine fmaf in f32, 10 u peS.  Output: the f32 add attention + pe and the store, u_out = 2^-23 (f32; as conv_bound) or
    2^-8 + 2^-23 (bf16, round to nearest even).
    Underflow: a weight below 2^-126 may be flushed; next to the maximum's weight 1 that is an absolute 2^-126 |v| per key, which with
    |v| < 2^10 and N < 2^16 stays below the 2^-100 floor.
    No element is excluded and no term is tied to the largest output."""
    A, Sqk, peS, ref = r["A"], r["Sqk"], r["peS"], r["out"]
    if kind == "scalar":
        P = psa_part_keys(N)
        Ew = 1.01 * (33 + 2) * U24 * Sqk + (P + 1) * EXPF_REL
        c_acc = 4 * P + 11
        extra = 0.0
    else:
        assert kind == "mfma", kind
        nb = -(-N // PSA_KB)
        Ew = 1.01 * (35 + 2) * U24 * Sqk + nb * EXP2_REL
        c_acc = 83 * nb + 4
        extra = 1.01 * 2.0 ** -8 * A
    u_out = 2.0 ** -23 if out_dtype == torch.float32 else 2.0 ** -8 + 2.0 ** -23
    return 2.02 * Ew * A + 1.01 * c_acc * U24 * A + extra + 1.01 * 10 * U24 * peS + u_out * ref.abs() + 2.0 ** -100


# ---------------------------------------------------------------------------------------------------------------------
# input families (fixed seeds; values the storage type holds exactly)
# ---------------------------------------------------------------------------------------------------------------------
DW_FAMILIES = ("uniform", "saturated", "impulse")
CONVT_FAMILIES = ("uniform", "impulse")
PSA_FAMILIES = ("uniform", "rising", "falling", "negative", "large", "tail", "impulse_v")


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape: torch.rand(*shape, generator=g) * 2 - 1


def _impulse_x(n, c, h, w, right_edge=False):
    x = torch.zeros(n, c, h, w)
    pos = impulse_positions(h, w)
    if right_edge:  # the edge pixel on the right border, mid height: its row-major neighbour is the next row's first pixel
        pos[1] = (h // 2, w - 1)
    for i in range(n):
        py, px = pos[i % 4]
        x[i, :, py, px] = (1 + (torch.arange(c) + i) % 7).float() * 0.25 * (1 if i % 2 == 0 else -1)
    return x


def dw_family(family, n, c, h, w, dtype, seed):
    """(x NCHW stored exactly in `dtype`, w9c (9, c) float32, bias (c) float32), built as conv_ref.conv_family builds its own:
      uniform    everything in [-1, 1];
      saturated  inputs * 40 and bias * 40, so the pre-activation spans about +-120: SiLU's tails, where __expf(-v) overflows;
      impulse    one nonzero pixel per image (corner, top edge, centre, far corner in turn), a different value per channel and image,
                 weights about (tap + 1) / 8: a wrong tap, border mask or image moves multiples of 1 / 8."""
    assert family in DW_FAMILIES, family
    U = _gen(seed)
    if family == "impulse":
        x = _impulse_x(n, c, h, w)
        wt = (torch.arange(9, dtype=torch.float32).view(9, 1) + 1) / 8 * (1 + 0.25 * U(9, c))
    else:
        x = U(n, c, h, w) * (40.0 if family == "saturated" else 1.0)
        wt = U(9, c)
    bias = U(c) * (40.0 if family == "saturated" else 1.0)
    return stored(x, dtype), wt.contiguous(), bias


def convt_family(family, n, cin, h, w, cout, dtype, seed):
    """(x NCHW, w (cin, cout, 2, 2), bias (cout) float32); x and w hold values `dtype` stores exactly (w rounded to nearest even, as
    the packer rounds).  impulse: one nonzero pixel per image, weights about (tap + 1) / 8 with tap = 2 i + j: a tap stored to the
    wrong one of the four output pixels moves multiples of 1 / 8."""
    assert family in CONVT_FAMILIES, family
    U = _gen(seed)
    if family == "impulse":
        x = _impulse_x(n, cin, h, w)
        wt = (torch.arange(4, dtype=torch.float32).view(1, 1, 2, 2) + 1) / 8 * (1 + 0.25 * U(cin, cout, 2, 2))
    else:
        x, wt = U(n, cin, h, w), U(cin, cout, 2, 2)
    return stored(x, dtype), stored(wt, dtype), U(cout)


def psa_family(family, n, h, w, heads, dtype, seed):
    """(qkv NHWC (n, h, w, heads * 128) stored exactly in `dtype`, pe_w9c (9, heads * 64) float32, pe_b float32) for scale = SCALE:
      uniform    q, k in [-2, 2], v in [-1, 1]: for N >= 64 the median over queries of the largest probability lies in (5 / N, 0.5);
      rising     k[j] = j / 8 in every dim, q about 8 step / (32 scale): logit = step * j (1 +- 0.01), step = max(0.5, 40 / (N - 1)),
                 strictly increasing in the key index, so the running maximum rises at every key of every block and partition;
      falling    the mirror image: the first key dominates and nothing rises after it;
      negative   every logit about -20 (q = c, k = -c (1 +- 0.1)), v about 3: a padded key let in at score 0 would take all the weight
                 and pull the output to 0;
      large      logits 60 t[j] with t a permutation of linspace(-1, 1, N): an unshifted exponential overflows / underflows;
      tail       k[N - 1] = 12 / (32 scale) in every dim, the other keys small, q about 1: the last key's weight is > 0.5;
      impulse_v  v nonzero at one pixel per image (corner, right edge at mid height, centre, far corner in turn), pe weights about (tap + 1) / 8, logits ~ 0 (near-flat
                 attention): pe's taps, its borders on 1 x W and H x 1 maps and the head's channel offset move multiples of 1 / 8."""
    assert family in PSA_FAMILIES, family
    U = _gen(seed)
    N, C = h * w, heads * HD
    q, k, v = U(n, N, heads, KD), U(n, N, heads, KD), U(n, N, heads, HD)
    pw, pb = U(9, C), U(C)
    idx = torch.arange(N, dtype=torch.float32).view(1, N, 1, 1)
    if family == "uniform":
        q, k = 2 * q, 2 * k
    elif family in ("rising", "falling"):
        step = max(0.5, 40.0 / max(N - 1, 1))
        q = 8 * step / (KD * SCALE) * (1 + 0.01 * q)
        k = ((idx if family == "rising" else N - 1 - idx) / 8).expand(n, N, heads, KD).clone()
    elif family == "negative":
        c = math.sqrt(20.0 / (KD * SCALE))
        q, k, v = torch.full_like(q, c), -c * (1 + 0.1 * k), 3 + 0.25 * v
    elif family == "large":
        c = math.sqrt(60.0 / (KD * SCALE))
        g = torch.Generator().manual_seed(seed + 1)
        t = (torch.linspace(-1, 1, N) if N > 1 else torch.ones(1))[torch.randperm(N, generator=g)].view(1, N, 1, 1)
        q, k = c * (1 + 0.01 * q), (c * t).expand(n, N, heads, KD).clone()
    elif family == "tail":
        q, k = 1 + 0.1 * q, 0.25 * k
        k[:, N - 1] = 12.0 / (KD * SCALE)
    else:
        q, k = 0.125 * q, 0.125 * k
        v = _impulse_x(n, C, h, w, right_edge=True).permute(0, 2, 3, 1).reshape(n, N, heads, HD)
        pw = (torch.arange(9, dtype=torch.float32).view(9, 1) + 1) / 8 * (1 + 0.25 * pw)
    qkv = torch.cat([q, k, v], dim=-1).reshape(n, h, w, heads * CH)
    return stored(qkv, dtype), pw.contiguous(), pb


# ---------------------------------------------------------------------------------------------------------------------
# the shapes both test files walk
# ---------------------------------------------------------------------------------------------------------------------
DW_MAPS = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (4, 4), (5, 4)]
DW_CHANNELS = [4, 6, 8, 12, 40]
PSA_MAPS = [(1, 1), (3, 5), (4, 4), (1, 17), (31, 1), (4, 8), (3, 11), (7, 9), (8, 8), (5, 13), (127, 1), (3, 43), (10, 20)]
PSA_HEADS = [1, 2, 3]
CONVT_MAPS = [(1, 1), (7, 9), (8, 8), (5, 13)]
CONVT_CH = {torch.float32: ([4, 12, 40], [4, 20, 40]), torch.bfloat16: ([8, 40, 72], [8, 24, 40])}


def dw_vector_width(c, dtype, offset=0):
    """The V of dwconv3_kernel<T, V, S> `upa_dwconv2d` launches for a view `offset` channels into buffers whose pitches and bases are
    multiples of 16 bytes: the 16-byte vector (f32 4, bf16 8) if c and the offset are multiples of it, else 1."""
    V = 8 if dtype == torch.bfloat16 else 4
    return V if c % V == 0 and offset % V == 0 else 1
