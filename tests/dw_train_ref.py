"""float64 reference of DWConv in train mode - depthwise 3x3 (stride 1, pad 1) + BatchNorm2d + SiLU | none - forward and backward, with
per-element bounds built from the operands only.  It is assembled from the pieces the project already pins: tests/train_ref.py
(BatchNorm sums, apply, the SiLU' term) and tests/psa_train_ref.py (the depthwise sums).  u = 2^-24.

The reference follows the stages of the computation, each on the operands that stage reads, so a bound never depends on a result of the
code under test:
  z        from x and w: 9 terms, (9 + 2) u sum |w x| and the store's rounding (2^-8 |z| in bf16);
  mean/var from the stored z: (terms + c0) u sum |terms| / npix, c0 = 0 | 1 (the square), the cancellation of E z^2 - mean^2, one f32
           store; `terms` is the longest float32 chain of the summation (64 in upa_bn_stats; a caller whose kernel sums otherwise
           passes its own count, from the shapes);
  running  (1 - m) r + m s with the unbiased variance: m times the bound of s and four roundings;
  y        from the stored z, mean, var: 4 C1 u M_y (train_ref.bn_act_fwd_ref) and the store;
  dgamma, dbeta, dz   from the stored z, mean, var and dy: (64 + c0) u sum |terms| and the SiLU' term 16 u sum |dy| (1 + |u|) for
           the sums; 4 C1 u (M_dz + T) and what the sums feed back for dz.  dz is held in float32 (`dz_dtype=F32`: it never leaves
           the workgroup) or stored once (`dz_dtype=BF16`: the composed form's rounding term);
  dx, dw   the depthwise sums of psa_train_ref.dw_bwd_ref on the float64 dz, plus the bound of dz CARRIED through the same taps:
           dx: sum |w| b_dz(shifted), dw: sum b_dz |x shifted|.
No element is excluded and no term is tied to the largest output."""

import torch

from tests import psa_train_ref as PR
from tests import train_ref as TR

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U24 = TR.U24
KERNEL_C1 = 4.0  # a kernel is allowed four times the float32 CPU restatement's constant (tests/test_hip_train_kernels.py)


def _store(t, dtype):
    return t if dtype == F64 else t.to(dtype).to(F64)


def _out_round(ref, arith, dtype):
    """The bound of a value computed to within `arith` and stored once in `dtype` (float64: not at all)."""
    if dtype == BF16:
        return arith + TR.half_ulp_bf16(ref.abs() + arith)
    return arith + (U24 * ref.abs() if dtype == F32 else 0.0)


def forward_ref(x, wt, gamma, beta, eps, act, running_mean=None, running_var=None, momentum=0.0, dtype=F32, z=None, mean=None, var=None,
                terms=64):
    """x (n, h, w, c), wt (c, 1, 3, 3).  `z`, `mean`, `var`: what the forward under test stored, when the later stages are to be
    referred to them; left out, the reference's own values rounded as the storage rounds them (nothing is rounded with dtype=F64).
    Returns a dict of references and bounds (b_*)."""
    n, h, w, c = x.shape
    npix = n * h * w
    r = {}
    r["z"], r["b_z"] = PR.dw_fwd_ref(x, wt, out_dtype=dtype if dtype != F64 else F32)
    zs = _store(r["z"], dtype) if z is None else z.to(F64)
    m, v, run, A1, A2 = TR.bn_stats_ref(zs.reshape(npix, c), running_mean, running_var, momentum)
    r["mean"], r["var"] = m, v
    dsum = 1.01 * terms * U24 * A1 / npix
    r["b_mean"] = dsum + U24 * m.abs() + 1e-300
    r["b_var"] = 1.01 * (terms + 1) * U24 * A2 / npix + 2 * m.abs() * dsum + dsum * dsum + U24 * v.abs() + 1e-300
    if run is not None:
        mom, unb = TR.f32(momentum), (npix / (npix - 1) if npix > 1 else 1.0)
        r["running_mean"], r["running_var"] = run
        r["b_running_mean"] = mom * r["b_mean"] + 4 * U24 * (running_mean.abs().to(F64) + m.abs()) + 1e-300
        r["b_running_var"] = mom * unb * r["b_var"] + 4 * U24 * (running_var.abs().to(F64) + unb * v.abs()) + 1e-300
    ms = (m if dtype == F64 else m.float().to(F64)) if mean is None else mean.to(F64)
    vs = (v if dtype == F64 else v.float().to(F64)) if var is None else var.to(F64)
    y, My = TR.bn_act_fwd_ref(zs.reshape(npix, c), ms, vs, gamma, beta, eps, act)
    r["y"] = y.reshape(n, h, w, c)
    r["b_y"] = _out_round(y, KERNEL_C1 * TR.C1_FWD_CPU * U24 * My, dtype).reshape(n, h, w, c) + 1e-300
    r["z_stored"], r["mean_stored"], r["var_stored"] = zs, ms, vs
    return r


def backward_ref(x, z, dy, wt, mean, var, gamma, beta, eps, act, dx0=None, dw0=None, dg0=None, db0=None, out_dtype=F32, dz_dtype=F32,
                 drop_xhat_mean=False, unflipped=False):
    """x, z, dy (n, h, w, c): the operands the backward reads (z, mean, var as the forward stored them).  Returns a dict: dz, dgamma,
    dbeta, dx, dw and their bounds.  Flags: the negative controls (mean(g xhat) omitted from dz; taps not flipped in dx)."""
    n, h, w, c = x.shape
    npix = n * h * w
    z2, dy2 = z.to(F64).reshape(npix, c), dy.to(F64).reshape(npix, c)
    dz, dgamma, dbeta, Mdz, Sb, Sg, T, Tb, Tg = TR.bn_act_bwd_ref(z2, dy2, mean, var, gamma, beta, eps, act)
    rstd, xh, _ = TR._bn_u(z2, mean, var, gamma, beta, eps)
    gr = gamma.to(F64) * rstd
    if drop_xhat_mean:
        dz = dz + gr * xh * dgamma / npix
    b_dg = 1.01 * (64 + 8) * U24 * Sg + 16 * U24 * Tg
    b_db = 1.01 * (64 + 2) * U24 * Sb + 16 * U24 * Tb
    feed = gr.abs() * (b_db + U24 * dbeta.abs() + xh.abs() * (b_dg + U24 * dgamma.abs())) / npix
    b_dz = _out_round(dz, KERNEL_C1 * TR.C1_BWD_CPU * U24 * (Mdz + T) + feed, dz_dtype if dz_dtype == BF16 else F64) + 1e-300
    r = dict(dz=dz.reshape(n, h, w, c), b_dz=b_dz.reshape(n, h, w, c))
    r["dgamma"], r["dbeta"] = dgamma + (dg0.to(F64) if dg0 is not None else 0.0), dbeta + (db0.to(F64) if db0 is not None else 0.0)
    r["b_dgamma"] = b_dg + U24 * dgamma.abs() + 2 * U24 * r["dgamma"].abs() + 1e-300
    r["b_dbeta"] = b_db + U24 * dbeta.abs() + 2 * U24 * r["dbeta"].abs() + 1e-300
    od = out_dtype if out_dtype != F64 else F32
    r["dx"], bdx, r["dw"], bdw = PR.dw_bwd_ref(x, r["dz"], wt, dx0, dw0, out_dtype=od, unflipped=unflipped)
    # the bound of dz through the taps (1.01: the sums' own roundings of the perturbed operands)
    ax, aw = x.to(F64).abs(), wt.to(F64).abs()
    ex, ew = torch.zeros_like(r["dz"]), torch.zeros(c, 1, 3, 3, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            ex += aw[:, 0, kh, kw] * PR._shift(r["b_dz"], -(kh - 1), -(kw - 1))
            ew[:, 0, kh, kw] = (r["b_dz"] * PR._shift(ax, kh - 1, kw - 1)).sum(dim=(0, 1, 2))
    r["b_dx"] = bdx + 1.01 * ex * (1.0 + (PR.HALF_BF16 if out_dtype == BF16 else U24))
    r["b_dw"] = bdw + 1.01 * ew + 2 * U24 * r["dw"].abs()
    return r


def train_f32(x, dy, wt, gamma, beta, eps, act, order):
    """The whole forward and backward in plain float32 on the CPU with every sum taken in `order` ("natural", "reversed", "partitioned"):
    z, mean, var, y, dgamma, dbeta, dx, dw."""
    n, h, w, c = x.shape
    npix = n * h * w
    z = PR.dw_f32(x, torch.zeros_like(x), wt, order)[0]

    def csum(t):
        t = t.reshape(npix, c)
        if order == "reversed":
            t = t.flip(0)
        elif order == "partitioned":
            t = torch.cat([t[1::2], t[0::2]])
        acc = torch.zeros(c, dtype=F64)
        for chunk in t.split(64):  # float32 inside a chunk of 64, float64 across (the project's reductions)
            part = torch.zeros(c)
            for row in chunk:
                part = part + row
            acc = acc + part.to(F64)
        return acc
    mean = (csum(z) / npix).float()
    var = (csum(z * z) / npix - mean.to(F64) ** 2).clamp_min(0).float()
    z2, dy2 = z.reshape(npix, c), dy.float().reshape(npix, c)
    y = TR.bn_fwd_f32(z2, mean, var, gamma, beta, eps, act).reshape(n, h, w, c)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    xh = (z2 - mean) * rstd
    u = gamma.float() * xh + beta.float()
    du = dy2
    if act == TR.ACT_SILU:
        s = 1.0 / (1.0 + torch.exp(-u))
        du = du * (s * (1.0 + u * (1.0 - s)))
    s0, s1 = csum(du), csum(du * xh)
    dz = TR.bn_bwd_f32(z2, dy2, mean, var, gamma, beta, eps, act, s0, s1).reshape(n, h, w, c)
    _, dx, dw = PR.dw_f32(x, dz, wt, order)
    return dict(z=z, mean=mean, var=var, y=y, dgamma=s1.float(), dbeta=s0.float(), dz=dz, dx=dx, dw=dw)
