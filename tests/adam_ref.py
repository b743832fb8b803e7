"""CPU reference of the fused Adam / AdamW step (upa_adam_ema, csrc/train.hip) - test infrastructure, never on the product path.

`adam_ref` does ONE step in float64 from float32 state, the way tests/train_ref.sgd_ref does for SGD: clip_grad_norm_ (+ GradScaler
unscale / skip), torch's `_single_tensor_adam` without amsgrad / maximize / capturable scaling, ModelEMA.update, zero_grad.  The
hyper-parameters are taken as given (Python floats): a caller that compares with the kernel passes the float32 values the C ABI
receives (`TR.f32`), a caller that compares with torch's own run passes torch's doubles - no hidden difference in beta or lr.
`adam_bounds` turns the magnitudes the reference returns into a per-element error bound of the float32 kernel, `auto_rule` restates
the reference's `optimizer=auto` choice (engine/trainer.py:908-917).
"""

from __future__ import annotations

import math

import torch

from tests import train_ref as TR

F64 = torch.float64
U24 = TR.U24


def auto_rule(nc, iterations):
    """(name, lr, momentum, warmup_bias_lr) of `build_optimizer(name="auto")`."""
    if iterations > 10000:
        return "SGD", 0.01, 0.9, 0.0
    return "AdamW", round(0.002 * 5 / (4 + nc), 6), 0.9, 0.0


def adam_ref(p, g, m, v, ema, sumsq, max_norm, lr, beta1, beta2, eps, wd, decoupled, t, ema_d, zero_grad, scale=None):
    """One step.  p, g, m, v, ema: float32 tensors (ema may be None); t: the step count AFTER this step's increment (>= 1; unused on a
    skipped step); under a GradScaler (`scale`) g and sumsq belong to the scaled gradients and a non-finite sumsq skips the step.
    Returns (p', g', m', v', ema' or None) in float64 and the terms `adam_bounds` needs."""
    p64, g64, m64, v64 = p.to(F64), g.to(F64), m.to(F64), v.to(F64)
    inv = 1.0 if scale is None else 1.0 / scale
    skip = scale is not None and not math.isfinite(sumsq)
    T = dict(skip=skip, d=ema_d, has_ema=ema is not None, p=p64)
    pn, mn, vn = p64, m64, v64
    if not skip:
        total = math.sqrt(sumsq) * inv
        coef = min(1.0, TR.f32(max_norm) / (total + TR.f32(1e-6))) * inv
        gc = g64 * coef
        if decoupled:
            decay = 1.0 - lr * wd
            p1, gi, wdp = p64 * decay, gc, torch.zeros_like(p64)
        else:
            decay = 1.0
            p1, gi, wdp = p64, gc + wd * p64, wd * p64
        w = 1.0 - beta1
        mn = m64 + (gi - m64) * w
        vn = v64 * beta2 + (1.0 - beta2) * gi * gi
        s = math.sqrt(1.0 - beta2 ** t)
        step = lr / (1.0 - beta1 ** t)
        q = vn.sqrt() / s
        denom = q + eps
        r = step * mn / denom
        pn = p1 - r
        T.update(gc=gc, wdp=wdp, wd=(0.0 if decoupled else wd), decay=decay, p1=p1, g=gi, m=m64, v=v64, w=w, beta2=beta2, mn=mn, vn=vn,
                 s=s, step=step, q=q, eps=eps, denom=denom, r=r)
    en = None
    if ema is not None:
        e64 = ema.to(F64)
        en = e64 * ema_d + (1.0 - ema_d) * pn
        T.update(e_d=e64 * ema_d, p_d=(1.0 - ema_d) * pn)
    T.update(pn=pn)
    return (pn, torch.zeros_like(g64) if zero_grad else g64, mn, vn, en), T


def adam_bounds(T, prev):
    """Per-element bounds (em, ev, ep, ee) on |kernel - reference| after one step, from the terms T of `adam_ref` and the bounds `prev`
    on the state the step started from (the gradient is the same float32 input on both sides).  u = 2**-24 bounds the relative error
    of one rounded float32 operation (the library is built without contraction and with correctly rounded divide / sqrt); a scalar that
    the kernel - or torch, which the same bound is used against - rounds to float32 counts as one operation on every term it multiplies;
    second-order terms in u are dropped, as in `_sgd_bounds`, except where a division by a perturbed quantity makes them matter.
    By the kernel's lines (adam_elem):
      gradient  coef = min(1, max_norm / (float(sqrt(ss)) inv_scale + 1e-6)) inv_scale: sqrt, cast, add, divide = 4 as in `_sgd_bounds`
                (a GradScaler's scale is a power of two - 2**16 times factors 2 and 0.5 - so 1 / scale and the products by it are
                exact), g coef = 1 more, Adam's + wd p one more: 6 u |g coef|; wd p itself: product and add, 2 u |wd p|; wd ep carried:
                                                        eg = wd ep + 6 u |g coef| + 2 u |wd p|
      decay     AdamW's p (1 - lr wd): the scalar and the product, carried ep scaled by |decay| <= 1:      ep1 = ep + 2 u |p decay|
      lerp      m' = m + (g - m) w is m (1 - w) + g w exactly, so the carried errors enter as (1 - w) em + w eg; roundings: w,
                the subtraction and the product act on w (|g| + |m|) >= w |g - m|, the add on |m'|:          em' = (1 - w) em + w eg + u (3 w (|g| + |m|) + |m'|)
      second    v beta2: scalar + product, 2 u |v beta2|; ((1 - beta2) g) g: scalar + two products, 3 u (1 - beta2) g^2; the add u |v'|
      moment    = u (|v beta2| + (1 - beta2) g^2); the gradient's error enters as (1 - beta2)(2 |g| eg + eg^2):
                                                        ev' = beta2 ev + (1 - beta2)(2 |g| eg + eg^2) + u (3 |v beta2| + 4 (1 - beta2) g^2)
      denom     |sqrt(v^) - sqrt(v')| = |v^ - v'| / (sqrt(v^) + sqrt(v')) <= ev' / (sqrt(v') + sqrt(max(v' - ev', 0))) =: es - a relative
                error in v' enters halved once ev' << v'; sqrt, the scalar sqrt(bc2) and the divide: 3 u q; eps as a float32 and the add:
                u eps + u denom:                                                        ed = es / sqrt(bc2) + u (4 q + 2 eps)
      update    r = (step m') / denom: the scalar step, product, divide: 3 u |r|; carried: step em' / (denom - ed) for the numerator,
                |r| ed / (denom - ed) for the denominator (|a/d^ - a/d| = |a| |d - d^| / (d d^)); the subtraction: u |p'|:
                                                        ep' = ep1 + (step em' + |r| ed) / (denom - ed) + u (3 |r| + |p'|)
      EMA       e d + (1 - d) p': product, 1 - d, product, add = 4 on both terms, as upa_sgd_nesterov_ema:  ee' = d ee + (1 - d) ep' + 4 u (|e d| + |(1 - d) p'|)
    A skipped step moves the EMA only (ep' = ep, em' = em, ev' = ev).  Where g = 0 and v = 0 exactly, ev' = 0 and denom = eps."""
    em, ev, ep, ee = prev
    u = U24
    if not T["skip"]:
        gc, wdp, g = T["gc"].abs(), T["wdp"].abs(), T["g"].abs()
        eg = T["wd"] * ep + 6 * u * gc + 2 * u * wdp
        ep1 = ep + 2 * u * T["p1"].abs() if T["decay"] != 1.0 else ep
        w, b2 = T["w"], T["beta2"]
        em = (1 - w) * em + w * eg + u * (3 * w * (g + T["m"].abs()) + T["mn"].abs())
        vb, gg = (T["v"] * b2).abs(), (1 - b2) * g * g
        ev = b2 * ev + (1 - b2) * (2 * g * eg + eg * eg) + u * (3 * vb + 4 * gg)
        vn = T["vn"]
        lo = (vn - ev).clamp_min(0.0).sqrt() + vn.sqrt()
        es = torch.where(ev > 0, ev / lo.clamp_min(1e-300), torch.zeros_like(ev))
        ed = es / T["s"] + u * (4 * T["q"] + 2 * T["eps"])
        room = T["denom"] - ed
        assert bool((room > 0).all()), "the bound on denom reaches denom itself: no bound on the update"
        r = T["r"].abs()
        ep = ep1 + (T["step"] * em + r * ed) / room + u * (3 * r + T["pn"].abs())
    if T["has_ema"]:
        d = T["d"]
        ee = d * ee + (1 - d) * ep + 4 * u * (T["e_d"].abs() + T["p_d"].abs())
    return em, ev, ep, ee


def carry(prev, outs, has_ema=True):
    """The bounds after the reference's state was rounded to float32 for its next step: + u |value| each."""
    pn, _, mn, vn, en = outs
    em, ev, ep, ee = prev
    return em + U24 * mn.abs(), ev + U24 * vn.abs(), ep + U24 * pn.abs(), ee + (U24 * en.abs() if has_ema and en is not None else 0.0)


def zeros(n):
    return tuple(torch.zeros(n, dtype=F64) for _ in range(4))
