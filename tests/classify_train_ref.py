"""Float64 CPU restatements of the classification-training kernels of csrc/classify_train.hip (global average pool forward and
backward, fused cross-entropy with its gradient, nn.Linear backward), each with the magnitude term its error bound is built from and
the number of rounded float32 operations on the kernel's path to one output, as tests/train_ref.py does for csrc/train.hip.

Plain torch on the CPU; nothing here imports the HIP package.  tests/test_classify_train_ref.py pins these functions against torch
autograd in float64; tests/test_hip_classify_train.py compares the kernels with them:
    |kernel - reference| <= (ops + SLACK) * 2**-24 * magnitude   (+ half a bf16 ulp of the reference where the output is bf16)
"""

import torch

F64 = torch.float64
U24 = 2.0 ** -24
UNDERFLOW = 2.0 ** -126  # the smallest normal float32: what ONE underflowing operation can lose, gradual or flushed.  A relative bound
# cannot hold below it: exp(z - max) of a far-off class (+-80 logits: exp(-150)) is below the float32 range while float64 keeps it.
SLACK = 2  # stated constant: the float32 rounding of the inputs' float64 reference itself and one guard operation

POOL_SLICES = 8    # csrc/classify_train.hip: pixel slices of an avgpool_fwd workgroup
CE_THREADS = 256   # ... threads of a cross-entropy workgroup (one row)


def avg_pool_ref(x):
    """x (n, c, h, w).  pooled (n, c) = mean over h, w; magnitude A = sum |x| / (h w).
    ops: a slice adds ceil(hw / 8) values, 7 additions join the slices, one divide."""
    x = x.to(F64)
    hw = x.shape[2] * x.shape[3]
    ops = -(-hw // POOL_SLICES) + (POOL_SLICES - 1) + 1
    return x.mean((2, 3)), x.abs().sum((2, 3)) / hw, ops


def avg_pool_bwd_ref(dpooled, h, w, prev=None):
    """dy (n, c, h, w) = dpooled / (h w) (+ prev); magnitude |dpooled| / (h w) + |prev|.  ops: one divide (+ one addition)."""
    d = dpooled.to(F64)[:, :, None, None].expand(-1, -1, h, w) / (h * w)
    mag = d.abs()
    ops = 1
    if prev is not None:
        d, mag, ops = d + prev.to(F64), mag + prev.to(F64).abs(), 2
    return d, mag, ops


def cross_entropy_ref(z, t, scale=1.0):
    """z (rows, nc), t (rows,) in [0, nc).  Returns loss (mean over rows of logsumexp(z) - z[t]), dz = (softmax - onehot) scale / rows
    and, for the bounds:
      mag_dz  = (softmax + onehot) scale / rows                       per element
      ops_dz  per row: see below
      mag_loss = mean over rows of (|max| + |log s| + |z_t| + 1)      (the 1: an error of s relative to s is absolute on log s)
      ops_loss
    Derivation (units of 2**-24, u = half an ulp relative):  with D = max_j |z_j - max| of the row,
      * z_j - max is one rounded subtraction, an absolute error <= D u, which exp turns into a RELATIVE error <= D u;
        expf itself is within 1 ulp = 2 u:  every term of s carries <= (D + 2) u;
      * the sum s of positive terms adds its depth: ceil(nc / 256) per thread + 6 butterfly steps + 3 waves;
        rel(s) <= D + 2 + depth;
      * p = exp / s: the numerator's D + 2, rel(s), one divide; p - onehot and / rows: one rounding each of a value <= p + onehot:
        ops_dz = 2 (D + 2) + depth + 3.   The scale is a power of two in every use (exact).
        exp(z_j - max) may underflow (s >= 1, so the quotient does not amplify it, and / rows only shrinks it): the gradient bound
        carries the absolute floor UNDERFLOW * scale next to the relative term.
      * row loss = (max + log s) - z_t: rel(s) absolute on log s, logf within 1 ulp (2 u) of |log s|, two roundings of sums bounded by
        the magnitude; the mean adds ceil(rows / 64) + 63 additions and a divide:
        ops_loss = (D_max + 2 + depth) + 2 + 2 + ceil(rows / 64) + 64."""
    z = z.to(F64)
    rows, nc = z.shape
    idx = torch.arange(rows)
    m = z.max(1).values
    e = torch.exp(z - m[:, None])
    s = e.sum(1)
    p = e / s[:, None]
    onehot = torch.zeros_like(z)
    onehot[idx, t.long()] = 1.0
    zt = z[idx, t.long()]
    row_loss = (m + torch.log(s)) - zt
    loss = row_loss.mean()
    dz = (p - onehot) * scale / rows
    D = (z - m[:, None]).abs().max(1).values
    depth = -(-nc // CE_THREADS) + 6 + 3
    ops_dz = 2 * (D + 2) + depth + 3
    mag_dz = (p + onehot) * scale / rows
    mag_loss = (m.abs() + torch.log(s).abs() + zt.abs() + 1.0).mean()
    ops_loss = float(D.max()) + 2 + depth + 4 + -(-rows // 64) + 64
    return loss, dz, mag_dz, ops_dz, mag_loss, ops_loss


def linear_bwd_ref(x, dy, w, dw_prev=None, db_prev=None):
    """x (m, k), dy (m, n), w (n, k).  dW = dy^T x, db = sum_m dy, dx = dy W (+ previous values for `accumulate`).
    Magnitudes: sum of |terms|.  ops: an FMA chain of m (dW, db) or n (dx) roundings, + 1 for the accumulate addition."""
    x, dy, w = x.to(F64), dy.to(F64), w.to(F64)
    m, n = dy.shape
    dw, db, dx = dy.t() @ x, dy.sum(0), dy @ w
    mag_dw, mag_db, mag_dx = dy.abs().t() @ x.abs(), dy.abs().sum(0), dy.abs() @ w.abs()
    ops_w = m
    if dw_prev is not None:
        dw, mag_dw = dw + dw_prev.to(F64), mag_dw + dw_prev.to(F64).abs()
        db, mag_db = db + db_prev.to(F64), mag_db + db_prev.to(F64).abs()
        ops_w = m + 1
    return dw, db, dx, mag_dw, mag_db, mag_dx, ops_w, n


def bound(ops, mag, ref=None, bf16=False):
    """(ops + SLACK) 2**-24 magnitude (+ half a bf16 ulp at the largest value the arithmetic bound allows, where the output is stored
    as bf16: tests/train_ref.half_ulp_bf16)."""
    b = (ops + SLACK) * U24 * mag
    if bf16:
        from tests.train_ref import half_ulp_bf16
        b = b + half_ulp_bf16(ref.abs() + b)
    return b
