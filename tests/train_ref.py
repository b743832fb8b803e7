"""Float64 CPU restatements of the training-step kernels of csrc/train.hip (BatchNorm statistics / apply / backward, the data and
weight gradients of a convolution, MaxPool2d and nearest-upsample backward, clip + SGD-Nesterov + EMA, GradScaler.update), each
with the magnitude term its error bound is built from, and the input families both test files use.

Plain torch on the CPU; nothing here imports the HIP package.  tests/test_train_ref.py pins these functions against torch autograd
in float64; tests/test_hip_train_kernels.py compares the kernels with them.  The BatchNorm functions work on (npix, c) matrices
(what an NHWC view is to those kernels), the convolution and pooling functions on NCHW."""

import math

import torch

from tests.conv_ref import stored  # noqa: F401  (the values a buffer of `dtype` really stores, as float32)

F64 = torch.float64
ACT_NONE, ACT_SILU = 0, 1  # UPA_ACT_* of include/upa.h
U24 = 2.0 ** -24


def f32(v):
    """The float64 value of the float32 nearest to v (scalars the C ABI takes as `float`)."""
    return float(torch.tensor(v, dtype=torch.float32))


def reduce_grid(npix):
    """csrc/train.hip reduce_grid: blocks of the channel reductions (64 pixels per block, at most 512 - 1024 beyond 1.5 M pixels)."""
    cap = 1024 if npix > 1500000 else 512
    return max(1, min(cap, -(-npix // 64)))


def sigmoid64(u):
    return 1.0 / (1.0 + torch.exp(-u))


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------
def bn_stats_ref(z, running_mean=None, running_var=None, momentum=0.0):
    """z (npix, c).  Returns mean, biased variance, (running_mean', running_var') or None, and the magnitude terms A1 = sum |z|,
    A2 = sum z^2 per channel.  The running update takes the unbiased estimate (npix > 1) as nn.BatchNorm2d does."""
    z = z.to(F64)
    n = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    run = None
    if running_mean is not None:
        unb = var * n / (n - 1) if n > 1 else var
        m = f32(momentum)
        run = ((1.0 - m) * running_mean.to(F64) + m * mean, (1.0 - m) * running_var.to(F64) + m * unb)
    return mean, var, run, z.abs().sum(0), (z * z).sum(0)


def _bn_u(z, mean, var, gamma, beta, eps):
    rstd = 1.0 / torch.sqrt(var.to(F64) + f32(eps))
    xh = (z.to(F64) - mean.to(F64)) * rstd
    return rstd, xh, gamma.to(F64) * xh + beta.to(F64)


def bn_act_fwd_ref(z, mean, var, gamma, beta, eps, act, residual=None):
    """y = act(gamma * (z - mean) / sqrt(var + eps) + beta) (+ residual) and the magnitude term
    M_y = L (|gamma rstd| (|z| + |mean|) + |beta|) + |residual|, L = 1.1 the largest slope of SiLU (1 without it)."""
    rstd, xh, u = _bn_u(z, mean, var, gamma, beta, eps)
    y = u * sigmoid64(u) if act == ACT_SILU else u
    M = (1.1 if act == ACT_SILU else 1.0) * ((gamma.to(F64) * rstd).abs() * (z.to(F64).abs() + mean.to(F64).abs()) + beta.to(F64).abs())
    if residual is not None:
        y = y + residual.to(F64)
        M = M + residual.to(F64).abs()
    return y, M


def bn_act_bwd_ref(z, dy, mean, var, gamma, beta, eps, act):
    """du = dy * act'(u); dbeta = sum du; dgamma = sum du xhat; dz = gamma rstd (du - (dbeta + xhat dgamma) / npix).
    Returns dz, dgamma, dbeta, M_dz = |gamma rstd| (|du| + (|sum du| + |xhat| |sum du xhat|) / npix), S_beta = sum |du|,
    S_gamma = sum |du xhat|, and the derivative's own term: SiLU'(u) passes through zero (u = -1.278), so a rounding error of the
    derivative scales with |dy| (1 + |u|), not with |du| - T = |gamma rstd| |dy| (1 + |u|) per element (0 without SiLU) and its sums
    T_beta = sum |dy| (1 + |u|), T_gamma = sum |dy| (1 + |u|) |xhat|."""
    rstd, xh, u = _bn_u(z, mean, var, gamma, beta, eps)
    du = dy.to(F64)
    t = torch.zeros_like(du)
    if act == ACT_SILU:
        s = sigmoid64(u)
        t = du.abs() * (1.0 + u.abs())
        du = du * (s * (1.0 + u * (1.0 - s)))
    n = z.shape[0]
    dbeta, dgamma = du.sum(0), (du * xh).sum(0)
    gr = gamma.to(F64) * rstd
    dz = gr * (du - (dbeta + xh * dgamma) / n)
    M = gr.abs() * (du.abs() + (dbeta.abs() + xh.abs() * dgamma.abs()) / n)
    return dz, dgamma, dbeta, M, du.abs().sum(0), (du * xh).abs().sum(0), gr.abs() * t, t.sum(0), (t * xh.abs()).sum(0)


def bn_fwd_f32(z, mean, var, gamma, beta, eps, act, residual=None):
    """bn_apply_kernel<T, false> in plain float32 on the CPU, its operation order (torch.exp and the IEEE divide for the
    transcendental): what the kernels' constant c1 is measured with."""
    f = torch.float32
    z, mean, var, gamma, beta = (t.to(f) for t in (z, mean, var, gamma, beta))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=f))
    u = gamma * ((z - mean) * rstd) + beta
    r = u / (1.0 + torch.exp(-u)) if act == ACT_SILU else u
    if residual is not None:
        r = r + residual.to(f)
    return r


def bn_bwd_f32(z, dy, mean, var, gamma, beta, eps, act, s0, s1):
    """bn_apply_kernel<T, true> in plain float32: k0, k1 are the float64 sums rounded to float32, inv = 1 / (float) npix."""
    f = torch.float32
    z, dy, mean, var, gamma, beta = (t.to(f) for t in (z, dy, mean, var, gamma, beta))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=f))
    xh = (z - mean) * rstd
    u = gamma * xh + beta
    du = dy
    if act == ACT_SILU:
        s = 1.0 / (1.0 + torch.exp(-u))
        du = du * (s * (1.0 + u * (1.0 - s)))
    inv = torch.tensor(1.0, dtype=f) / torch.tensor(float(z.shape[0]), dtype=f)
    return gamma * rstd * (du - (s0.to(f) + xh * s1.to(f)) * inv)


BN_FAMILIES = ("uniform", "poison", "offset", "constant", "impulse")


def bn_family(family, npix, c, dtype, seed):
    """(z, dy, residual, gamma, beta) as CPU float32 holding values `dtype` stores exactly; z, dy, residual are (npix, c).
      uniform   z, dy in [-1, 1];
      poison    the same payload (the caller fills the neighbouring channels of the views with NaN);
      offset    z = 100 + noise of 1 / 8: E[z^2] - mean^2 cancels seven digits;
      constant  z the same value in every pixel of a channel: var = 0, rstd = 1 / sqrt(eps);
      impulse   dy nonzero in two pixels only: the very last one, and the last pixel of the first block's chunk of the reduction -
                where the kernel's prefetch runs past the chunk and has to mask what it fetched."""
    assert family in BN_FAMILIES, family
    g = torch.Generator().manual_seed(seed)

    def U(*shape):
        return torch.rand(*shape, generator=g) * 2 - 1
    z, dy = U(npix, c), U(npix, c)
    if family == "offset":
        z = 100.0 + z / 8
    elif family == "constant":
        z = (U(1, c) * 3).expand(npix, c).clone()
    elif family == "impulse":
        chunk = -(-npix // reduce_grid(npix))
        keep = torch.zeros(npix, 1)
        keep[npix - 1] = 1.0
        keep[min(chunk, npix) - 1] = 1.0
        dy = (dy + 2.0 * torch.sign(dy)) * keep
    gamma, beta = 0.5 + torch.rand(c, generator=g), U(c) * 0.3
    return stored(z, dtype), stored(dy, dtype), stored(U(npix, c), dtype), gamma, beta


# ---------------------------------------------------------------------------------------------------------------------
# convolution gradients
# ---------------------------------------------------------------------------------------------------------------------
def dgrad_ref(dz, w, stride, pad, hw):
    """Data gradient of conv2d(x, w, stride, pad) for an (h, w) input as an explicit scatter over the taps:
    dx[n, ci, oy s + kh - p, ox s + kw - p] += dz[n, co, oy, ox] w[co, ci, kh, kw].  Returns dx and S = the same sum over |dz| |w|."""
    h, wd = hw
    n, cout, oh, ow = dz.shape
    k = w.shape[2]
    cin = w.shape[1]
    dz64, w64 = dz.to(F64), w.to(F64)
    out = []
    for a, b in ((dz64, w64), (dz64.abs(), w64.abs())):
        big = torch.zeros(n, cin, (oh - 1) * stride + k + 2 * pad + stride, (ow - 1) * stride + k + 2 * pad + stride, dtype=F64)
        for kh in range(k):
            for kw in range(k):
                t = torch.einsum("nohw,oi->nihw", a, b[:, :, kh, kw])
                big[:, :, kh:kh + (oh - 1) * stride + 1:stride, kw:kw + (ow - 1) * stride + 1:stride] += t
        out.append(big[:, :, pad:pad + h, pad:pad + wd].clone())
    return out[0], out[1]


def wgrad_ref(x, dz, k, stride, pad):
    """dW[co, ci, kh, kw] = sum over n, oy, ox of dz[n, co, oy, ox] x[n, ci, oy s + kh - p, ox s + kw - p]; S on absolute operands."""
    n, cin, h, w = x.shape
    _, cout, oh, ow = dz.shape
    out = []
    for a, b in ((x.to(F64), dz.to(F64)), (x.to(F64).abs(), dz.to(F64).abs())):
        xp = torch.zeros(n, cin, h + 2 * pad + stride, w + 2 * pad + stride, dtype=F64)
        xp[:, :, pad:pad + h, pad:pad + w] = a
        dw = torch.zeros(cout, cin, k, k, dtype=F64)
        for kh in range(k):
            for kw in range(k):
                xs = xp[:, :, kh:kh + (oh - 1) * stride + 1:stride, kw:kw + (ow - 1) * stride + 1:stride]
                dw[:, :, kh, kw] = torch.einsum("nohw,nihw->oi", b, xs)
        out.append(dw)
    return out[0], out[1]


def phase_weights_ref(w):
    """upa_dgrad_s2_phase_weights restated from its comment: V[ph][ci][co][a][b] = W[co][ci][kh][kw], ph = 2 py + px,
    py = 0: a = 0 -> kh = 1, a = 1 -> none; py = 1: a = 0 -> kh = 2, a = 1 -> kh = 0 (kw from px, b alike); zero where a parity has no tap."""
    cout, cin = w.shape[:2]
    v = torch.zeros(4, cin, cout, 2, 2, dtype=w.dtype)
    tap = {0: {0: 1}, 1: {0: 2, 1: 0}}
    for py in (0, 1):
        for px in (0, 1):
            for a, kh in tap[py].items():
                for b, kw in tap[px].items():
                    v[2 * py + px, :, :, a, b] = w[:, :, kh, kw].t()
    return v


# ---------------------------------------------------------------------------------------------------------------------
# pooling / upsampling backward
# ---------------------------------------------------------------------------------------------------------------------
def maxpool_bwd_ref(x, dy, k, s, p):
    """MaxPool2d(k, s, p) backward: every window sends its dy to the FIRST maximum in row-major window order among the taps inside
    the image (strictly greater replaces; the first in-image tap is elected even when it holds -inf).  Returns dx and A = the sum of
    |dy| over the same terms, float64 NCHW."""
    n, c, h, w = x.shape
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    assert tuple(dy.shape) == (n, c, oh, ow), (dy.shape, (n, c, oh, ow))
    x64, dy64 = x.to(F64), dy.to(F64)
    dx = torch.zeros(n, c, h * w, dtype=F64)
    A = torch.zeros(n, c, h * w, dtype=F64)
    for oy in range(oh):
        for ox in range(ow):
            best = torch.full((n, c), -math.inf, dtype=F64)
            idx = torch.full((n, c), -1, dtype=torch.long)
            for kh in range(k):
                yy = oy * s - p + kh
                if yy < 0 or yy >= h:
                    continue
                for kw in range(k):
                    xx = ox * s - p + kw
                    if xx < 0 or xx >= w:
                        continue
                    v = x64[:, :, yy, xx]
                    up = (v > best) | (idx < 0)
                    best = torch.where(up, v, best)
                    idx = torch.where(up, torch.full_like(idx, yy * w + xx), idx)
            assert bool((idx >= 0).all()), "a window without a tap inside the image"
            dx.scatter_add_(2, idx.unsqueeze(2), dy64[:, :, oy, ox].unsqueeze(2))
            A.scatter_add_(2, idx.unsqueeze(2), dy64[:, :, oy, ox].abs().unsqueeze(2))
    return dx.view(n, c, h, w), A.view(n, c, h, w)


POOL_FAMILIES = ("ties", "flat", "neginf")


def pool_family(family, n, c, h, w, k, s, p, dtype, seed):
    """(x, dy) NCHW float32 holding values `dtype` stores exactly.
      ties    x quantised to 1 / 4: most windows hold their maximum several times;
      flat    x the same everywhere: every window elects its first tap inside the image;
      neginf  a quarter of x is -inf, and so are whole windows' worth of it: the top-left (k + s) x (k + s) corner of every channel
              and all of channel 1.
    dy is finite in every family: multiples of 1 / 128 in [-1, 1], which bf16 holds and whose sums of k^2 terms float32 adds without
    rounding - the float32 kernels are exact on them and the bf16 kernels round once."""
    assert family in POOL_FAMILIES, family
    g = torch.Generator().manual_seed(seed)
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x = ((torch.rand(n, c, h, w, generator=g) * 2 - 1) * 4).round() / 4
    if family == "flat":
        x = torch.full((n, c, h, w), 0.75)
    elif family == "neginf":
        x[torch.rand(n, c, h, w, generator=g) < 0.25] = -math.inf
        x[:, :, :k + s, :k + s] = -math.inf
        x[:, 1] = -math.inf
    dy = ((torch.rand(n, c, oh, ow, generator=g) * 2 - 1) * 128).round() / 128
    return stored(x, dtype), stored(dy, dtype)


def upsample2x_bwd_ref(dy):
    """Backward of the nearest 2x upsample: dx = the sum of each 2 x 2 block of dy; A = the same over |dy|."""
    d = dy.to(F64)
    n, c, h2, w2 = d.shape
    b = d.view(n, c, h2 // 2, 2, w2 // 2, 2)
    return b.sum((3, 5)), b.abs().sum((3, 5))


# ---------------------------------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------------------------------
def sumsq_ref(g):
    """sum g^2 exactly rounded (products of float32 are exact in float64, math.fsum adds them without error)."""
    return math.fsum((g.to(F64) ** 2).tolist())


def sgd_ref(p, g, buf, ema, sumsq, max_norm, lr, momentum, wd, first_step, ema_d, zero_grad, scale=None):
    """clip_grad_norm_ + SGD(nesterov) + ModelEMA.update + zero_grad on float32 state in float64 arithmetic; under a GradScaler
    (scale given) g and sumsq belong to the scaled gradients and a non-finite sumsq skips the parameter step.
    Returns (p', g', buf', ema' or None) as float64 and the magnitude terms (Mg, Mb, Mp, Me) of the four roundings."""
    p64, g64, b64 = p.to(F64), g.to(F64), buf.to(F64)
    max_norm, lr, momentum, wd, ema_d = (f32(v) for v in (max_norm, lr, momentum, wd, ema_d))
    inv = 1.0 if scale is None else 1.0 / scale
    skip = scale is not None and not math.isfinite(sumsq)
    z = torch.zeros_like(p64)
    pn, bn, Mg, Mb, Mp = p64, b64, z, z, p64.abs()
    if not skip:
        total = math.sqrt(sumsq) * inv
        coef = min(1.0, max_norm / (total + f32(1e-6))) * inv
        gi = g64 * coef + wd * p64
        Mg = (g64 * coef).abs() + (wd * p64).abs()
        bn = gi if first_step else momentum * b64 + gi
        Mb = Mg if first_step else (momentum * b64).abs() + Mg
        upd = gi + momentum * bn
        pn = p64 - lr * upd
        Mp = p64.abs() + lr * (Mg + momentum * Mb)
    en, Me = None, z
    if ema is not None:
        en = ema.to(F64) * ema_d + (1.0 - ema_d) * pn
        Me = (ema.to(F64) * ema_d).abs() + ((1.0 - ema_d) * pn).abs()
    return (pn, torch.zeros_like(g64) if zero_grad else g64, bn, en), (Mg, Mb, Mp, Me)


def scaler_ref(state, sumsq, growth, backoff, interval):
    """GradScaler.update() on the state [scale, growth tracker, found_inf, the scale before the update]."""
    scale, tracker = state[0], int(state[1])
    inf = not math.isfinite(sumsq)
    new = scale
    if inf:
        new, tracker = scale * f32(backoff), 0
    else:
        tracker += 1
        if tracker == interval:
            new, tracker = scale * f32(growth), 0
    return [f32(new), float(tracker), 1.0 if inf else 0.0, scale]


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_hip_train_kernels.py (tests/test_train_ref.py walks the same ones on the CPU)
# ---------------------------------------------------------------------------------------------------------------------
BN_CHANNELS = {torch.float32: (4, 48, 144, 1024), torch.bfloat16: (8, 80, 136, 2048)}
BN_NPIX = (1, 3, 63, 65, 257, 4099)
BN_EPS = 1e-3


def bn_cases(dtype, c):
    """(npix, family, act, accumulate, residual, running, seed) for one (dtype, c): every pixel count with every family (256 channel
    groups: the two largest pixel counts with `uniform` and `impulse` only); the four options walk through all sixteen combinations."""
    out = []
    for i, npix in enumerate(BN_NPIX):
        for j, family in enumerate(BN_FAMILIES):
            q = i * len(BN_FAMILIES) + j
            if c >= 1024 and npix >= 257 and family in ("poison", "offset", "constant"):
                continue  # the widest views keep the run short: these families meet the large pixel counts at the other widths
            out.append((npix, family, ACT_SILU if q & 1 else ACT_NONE, (q >> 1) & 1, bool((q >> 2) & 1), bool((q >> 3) & 1),
                        c * 1000 + q + (500 if dtype == torch.bfloat16 else 0)))
    return out


def half_ulp_bf16(x):
    """Half a bfloat16 ulp at magnitude |x| (float64): what one round-to-nearest into bf16 can move a value of that size."""
    e = torch.frexp(x.abs().to(F64).clamp_min(2.0 ** -126))[1]
    return torch.pow(torch.tensor(2.0, dtype=F64), (e - 9).to(F64))


# c1 of the BatchNorm apply kernels: the worst |float32 restatement - float64 reference| / (2^-24 M) over bn_cases of every (dtype, c),
# measured by tests/test_train_ref.py::test_c1_constants (which asserts these values still cover it); the kernels are allowed 4 x that
C1_FWD_CPU, C1_BWD_CPU = 5.0, 7.0  # measured 4.667 and 6.654

DGRAD_CHANNELS = ((16, 64), (24, 64), (40, 72), (64, 128))   # cin, cout
DGRAD_MAPS = ((13, 11), (16, 16), (7, 20))                   # dx (h, w)
WGRAD_CASES = (
    # dtype, cin, cout, k, stride, pad, the branch of upa_conv2d_wgrad's dispatch the shape takes
    (torch.float32, 20, 44, 3, 1, 1, "f32 <1,1>: wgrad_small (cin <= 32)"),
    (torch.float32, 36, 28, 1, 1, 0, "f32 <1,1>: wgrad_small (cout <= 32), k 1"),
    (torch.float32, 36, 44, 3, 2, 1, "f32 <2,2>: both above 32, stride 2"),
    (torch.float32, 132, 36, 1, 1, 0, "f32 <2,2>: k 1 with cout < 128"),
    (torch.float32, 132, 140, 1, 1, 0, "f32 <4,4>: k 1, cin and cout >= 128"),
    (torch.bfloat16, 16, 40, 1, 1, 0, "bf16 generic <1,1>: k 1 with cin < 32"),
    (torch.bfloat16, 40, 72, 1, 2, 0, "bf16 generic <2,2>: k 1 with stride 2"),
    (torch.bfloat16, 136, 136, 1, 2, 0, "bf16 generic <4,4>: k 1 with stride 2, cin and cout >= 128"),
)
WGRAD_MAP = (2, 9, 13)
POOL_KSP = ((5, 1, 2), (3, 1, 1), (2, 2, 0), (2, 1, 0), (3, 2, 1))
POOL_MAPS = ((1, 1), (2, 3), (4, 4), (9, 11), (8, 16))


def conv_grad_family(n, cin, cout, h, w, k, stride, pad, dtype, seed):
    """(x, dz, w) NCHW / OIHW float32 in [-1, 1] holding values `dtype` stores exactly."""
    g = torch.Generator().manual_seed(seed)
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    def U(*shape):
        return stored(torch.rand(*shape, generator=g) * 2 - 1, dtype)
    return U(n, cin, h, w), U(n, cout, oh, ow), U(cout, cin, k, k)
