"""Float64 CPU restatement of `upa_conv2d_bias_act` (csrc/conv.hip and the kernel families behind it) and the per-element error
bound its kernels are held to.

Plain torch on the CPU; nothing here imports the HIP package's kernels.  tests/test_conv_ref.py pins these functions (against a
seven-loop convolution, hand-worked pixels and an f32 emulation of the kernels' arithmetic); tests/test_hip_conv_views.py compares
every dispatch path with them."""

import torch
import torch.nn.functional as F

F64 = torch.float64
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2  # UPA_ACT_* of include/upa.h
U24 = 2.0 ** -24


def act_ref(v, act):
    """The activation in float64: SiLU as v / (1 + exp(-v)) (exp overflows to inf at v < -709: the quotient is then -0)."""
    if act == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    assert act == ACT_NONE, act
    return v


def conv_ref(x, w, bias, residual, k, stride, pad, act):
    """x: NCHW, w: OIHW (k x k), bias: (cout) or None, residual: NCHW of the output's shape or None - all holding values their storage
    type represents exactly.  Returns three float64 NCHW tensors:
      v    the pre-activation bias + sum x * w,
      S    |bias| + sum |x| * |w|: the same convolution on absolute operands (what a rounding error of the sum scales with),
      ref  act(v) + residual."""
    assert w.shape[2] == k and w.shape[3] == k and x.shape[1] == w.shape[1]
    x64, w64 = x.to(F64), w.to(F64)
    b64 = None if bias is None else bias.to(F64)
    v = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
    S = F.conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), stride=stride, padding=pad)
    ref = act_ref(v, act)
    if residual is not None:
        assert residual.shape == ref.shape, (residual.shape, ref.shape)
        ref = ref + residual.to(F64)
    return v, S, ref


def conv_bound(v, S, ref, K, act, out_dtype):
    """Per-element bound on |kernel - ref| for a kernel that multiplies exactly (bf16 x bf16, or f32 MFMA with fused rounding per
    step), accumulates K = cin * k * k products and the bias in float32 in any order, applies the activation in float32 and rounds
    once into `out_dtype`:

      L * 1.01 * (K + 1) * 2^-24 * S  +  (|v| + 6) * 2^-24 * |act(v)|  +  u_out * |ref|  +  2^-100

      accumulation  an f32 sum of K + 1 terms errs by at most (K + 1) 2^-24 S to first order, 1.01 covers the higher orders; the
                    activation passes it on times its largest slope L (SiLU: 1.0998 -> 1.1, ReLU / none: 1);
      activation    SiLU only: expf(-v) carries the rounding of v * log2(e), |v| 2^-24 relative, and the reciprocal or divide, the
                    add and the multiply six more units;
      output        u_out = 2^-8 for bf16 (round to nearest even), 2^-23 for f32 (the store and the residual add in f32).
    No element is excluded and no term is tied to the largest output."""
    lip = 1.1 if act == ACT_SILU else 1.0
    bound = lip * 1.01 * (K + 1) * U24 * S
    if act == ACT_SILU:
        bound = bound + (v.abs() + 6.0) * U24 * act_ref(v, act).abs()
    u_out = 2.0 ** -8 if out_dtype == torch.bfloat16 else 2.0 ** -23
    return bound + u_out * ref.abs() + 2.0 ** -100


# ---------------------------------------------------------------------------------------------------------------------
# input families (shared by tests/test_conv_ref.py and tests/test_hip_conv_views.py)
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("uniform", "poison", "saturated", "impulse", "impulse2")


def stored(t, dtype):
    """The values a buffer of `dtype` really stores, as float32."""
    return t.to(dtype).float()


def impulse_positions(h, w):
    """Corner, top edge, centre, far corner: where the impulse families put an image's one nonzero pixel, in turn."""
    return [(0, 0), (0, w // 2), (h // 2, w // 2), (h - 1, w - 1)]


def conv_family(family, n, cin, h, w, cout, k, dtype, seed, with_bias=True, with_res=False, out_hw=None):
    """(x NCHW, w OIHW, bias or None, residual NCHW or None) as CPU float32 holding values `dtype` stores exactly (the bias is float32
    in either mode).
      uniform    everything in [-1, 1];
      poison     the same payload (the caller fills the neighbouring channels of the input view with NaN);
      saturated  inputs and bias scaled so that the pre-activation spans about +-120 (standard deviation 40): SiLU's tails, where
                 expf(-v) overflows to inf and the product must come out as -0, and ReLU's clamp;
      impulse    one nonzero pixel per image - image i at impulse_positions[i % 4] (impulse2: [(i + 2) % 4]) - holding a different
                 value per channel and image, weights about (tap + 1) / 8: a wrong tap order, a wrong border mask or a leak from image
                 i into image i + 1 moves whole multiples of 1 / 8."""
    assert family in FAMILIES, family
    g = torch.Generator().manual_seed(seed)

    def U(*shape):
        return torch.rand(*shape, generator=g) * 2 - 1
    K = cin * k * k
    if family in ("impulse", "impulse2"):
        x = torch.zeros(n, cin, h, w)
        pos = impulse_positions(h, w)
        for i in range(n):
            py, px = pos[(i + (2 if family == "impulse2" else 0)) % 4]
            x[i, :, py, px] = (1 + (torch.arange(cin) + i) % 7).float() * 0.25 * (1 if i % 2 == 0 else -1)
        tap = torch.arange(k * k, dtype=torch.float32).view(1, 1, k, k)
        wt = (tap + 1) / 8 * (1 + 0.25 * U(cout, cin, k, k))
    else:
        x = U(n, cin, h, w)
        wt = U(cout, cin, k, k)
        if family == "saturated":
            x = x * (120.0 / K ** 0.5)
    bias = None
    if with_bias:
        bias = U(cout) * (40.0 if family == "saturated" else 1.0)
    res = None
    if with_res:
        assert out_hw is not None
        res = stored(U(n, cout, *out_hw), dtype)
    return stored(x, dtype), stored(wt, dtype), bias, res
