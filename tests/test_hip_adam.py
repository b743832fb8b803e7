"""-m gpu: upa_adam_ema and upa_adam_step_advance (csrc/train.hip) at the C ABI against the float64 step of tests/adam_ref.py.

Every element of the parameters, both moments and the EMA is held to `adam_ref.adam_bounds` - roundings counted in units of 2**-24 on
the magnitudes of each line of the kernel, the bound of the state a step started from carried through - over three steps; the
reference keeps its own float32 state, as in test_sgd_nesterov_ema.  Every buffer the kernels may write sits between guard words.
The hyper-parameters go to the reference as the float32 values the C ABI receives.

Gradients: exact zeros from the first step on (there v = 0 and denom = eps: the update must be finite and the parameter moves by decay
only); every other |g| lies in [1e-6, 1e2], and in [1e-3, 1e2] on the clipping step, so that g * g stays clear of float32's underflow
((1 - beta2) (g coef)^2 >= 1e-17) and a clipped |g| stays above 10 eps in the denominator: the float64 reference and the float32
kernel describe the same function, and no bound rests on a quantity float32 cannot hold."""

import math

import pytest
import torch

from tests import adam_ref as AR
from tests import kernel_check as KC
from tests import train_ref as TR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
UPA_EINVAL = -1
B1, B2, EPS = TR.f32(0.9), TR.f32(0.999), TR.f32(1e-8)
MAX_NORM = 10.0
LRS = [TR.f32(1e-3), TR.f32(5e-4), TR.f32(2e-3), TR.f32(1e-3)]


class Guarded:
    """A device array of `x` between `left` and `right` NaN guard words (left also sets the payload's offset from a 16-byte boundary)."""

    def __init__(self, x, left=4, right=4):
        DEV = KC.env()[0]
        self.n, self.left = x.numel(), left
        host = torch.full((left + self.n + right,), NAN, dtype=x.dtype) if x.dtype.is_floating_point else \
            torch.full((left + self.n + right,), -77, dtype=x.dtype)
        host[left:left + self.n] = x
        self.buf = host.to(DEV)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.left * self.buf.element_size()

    def get(self, what):
        a = self.buf.cpu()
        g = torch.cat([a[:self.left], a[self.left + self.n:]])
        held = torch.isnan(g) if a.dtype.is_floating_point else g == -77
        assert bool(held.all()), f"{what}: a guard word was written"
        return a[self.left:self.left + self.n].clone()

    def clone(self):
        c = Guarded.__new__(Guarded)
        c.n, c.left, c.buf = self.n, self.left, self.buf.clone()
        return c


def _gradient(n, gen, step, scale):
    """log-uniform magnitudes, random signs, exact zeros at i % 3 == 1; step 1 is the clipping step."""
    lo, hi = (-3.0, 2.0) if step == 1 else (-6.0, -2.0)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=F64) * (hi - lo) + lo)
    g = (mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).float()
    g[1::3] = 0.0
    nz = g[g != 0].abs()
    assert nz.numel() == 0 or (float(nz.min()) >= 0.99e-6 and float(nz.max()) <= 1.01e2)
    return g * (scale or 1.0)


def _call(lib, st, P, G, M, V, E, ss, lr, wd, decoupled, T, d, dd, zero, sstate, advance=True):
    L = KC.env()[1]
    if advance:
        L.check(lib.upa_adam_step_advance(T.ptr, ss.data_ptr(), None if sstate is None else sstate.data_ptr(), st), "adam_step_advance")
    L.check(lib.upa_adam_ema(P.ptr, G.ptr, M.ptr, V.ptr, None if E is None else E.ptr, P.n, ss.data_ptr(), MAX_NORM, lr, B1, B2, EPS, wd,
                             decoupled, T.ptr, d, None if dd is None else dd.data_ptr(), zero,
                             None if sstate is None else sstate.data_ptr(), st), "adam_ema")


# (decoupled, weight decay, ema, decay from device memory, zero_grad, loss scale, guard words in front of p, g, m, v, ema).
# Guards of 4: 16-byte aligned; equal guards of 1 or 2: the 16-byte groups behind a head of 3 / 2 elements; unequal: element by element.
COMBOS = [(1, 5e-4, True, False, 1, None, (4, 4, 4, 4, 4)),
          (0, 5e-4, True, True, 0, None, (1, 1, 1, 1, 1)),
          (1, 0.0, False, False, 0, None, (4, 4, 4, 4, 4)),
          (0, 0.0, True, False, 1, None, (4, 1, 2, 3, 4)),
          (1, 5e-4, True, True, 1, 1024.0, (2, 2, 2, 2, 2)),
          (0, 5e-4, True, False, 1, 1024.0, (4, 4, 4, 4, 4))]


@pytest.mark.parametrize("n", [1, 1000, 300001])
@KC.stop_after_fault
def test_adam_ema(n):
    """Three steps per combination of COMBOS (n = 1: one lane; 1000: a partial block; 300 001: more than one grid-stride trip) with the
    lr changed between the steps, a clipping step (1), the decay read from ema_d_dev while the scalar holds a wrong value, ema = NULL
    (the buffer must not move), zero_grad 0 and 1; after each call *step_dev is what upa_adam_step_advance left.  The first step of
    every combination runs twice from the same buffers and must agree bit for bit.  Scaled (scaler_state = {1024, ...}, gradients
    times 1024): lands on the unscaled step's bound; grad_sumsq = inf, then NaN: p, exp_avg, exp_avg_sq bit-identical, the count not
    advanced, the EMA moved, g zeroed; the next finite step takes the un-advanced t (4).
    Measured on MI355X, worst error / bound: 0.81 / 0.93 / 0.98 for n = 1 / 1000 / 300 001, each time a parameter, whose bound is led by
    the half ulp of its final subtraction."""
    DEV, L, lib, st = KC.env()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.rand(n, generator=gen) * 2 - 1
    report = []
    for decoupled, wd, with_ema, use_dev, zero, scale, guards in COMBOS:
        wd = TR.f32(wd)
        P, M, V, Em = p0.clone(), torch.zeros(n), torch.zeros(n), p0.clone()  # the reference's float32 state
        Pd, Md, Vd, Ed = Guarded(P, guards[0]), Guarded(M, guards[2]), Guarded(V, guards[3]), Guarded(Em, guards[4])
        Td = Guarded(torch.zeros(1, dtype=torch.int32), 1, 1)
        prev = AR.zeros(n)
        sstate = None if scale is None else torch.tensor([scale, 0.0, 0.0, 0.0], device=DEV)
        t = 0

        def one(step, ss, g, skipped=False):
            nonlocal P, M, V, Em, prev, t
            what = f"adam n{n} dec{decoupled} wd{wd:g} ema{int(with_ema)} dev{int(use_dev)} zero{zero} scale{scale} guards{guards} step{step}"
            d = 0.9999 * (1 - math.exp(-(step + 1) / 2000.0)) if step < 2 else 0.75
            d32 = TR.f32(d)
            Gd, ssd = Guarded(g, guards[1]), torch.tensor([ss], dtype=F64, device=DEV)
            dd = torch.tensor([d], device=DEV)
            args = (ssd, LRS[step], wd, decoupled, Td, 0.123 if use_dev else d, dd if use_dev else None, zero, sstate)
            if step == 0:  # two runs from the same buffers agree in every bit
                c = [x.clone() for x in (Pd, Gd, Md, Vd, Ed, Td)]
                _call(lib, st, c[0], c[1], c[2], c[3], c[4] if with_ema else None, *args[:4], c[5], *args[5:])
            before = (Pd.get(what), Md.get(what), Vd.get(what))
            _call(lib, st, Pd, Gd, Md, Vd, Ed if with_ema else None, *args)
            t += 0 if skipped else 1
            assert int(Td.get(what)[0]) == t, f"{what}: step count {int(Td.get(what)[0])}, expected {t}"
            got = (Pd.get(what), Gd.get(what), Md.get(what), Vd.get(what), Ed.get(what))
            if step == 0:
                for a, b in zip(got, c):
                    assert KC.same_bits(a, b.get(what)), what + ": two runs differ"
            outs, T = AR.adam_ref(P, g, M, V, Em if with_ema else None, ss, MAX_NORM, LRS[step], B1, B2, EPS, wd, decoupled, t, d32, zero, scale)
            pn, gn, mn, vn, en = outs
            if skipped:
                assert KC.same_bits(got[0], before[0]) and KC.same_bits(got[2], before[1]) and KC.same_bits(got[3], before[2]), \
                    what + ": p or a moment moved on a skipped step"
            else:
                nz = (T["gc"].abs())[g != 0]
                assert nz.numel() == 0 or float(nz.min()) >= 10 * EPS, "a clipped gradient is not clear of eps"
            prev = AR.adam_bounds(T, prev)
            KC.check_bound(got[2].double(), mn, prev[0] + 1e-300, what + " exp_avg", report)
            KC.check_bound(got[3].double(), vn, prev[1] + 1e-300, what + " exp_avg_sq", report)
            KC.check_bound(got[0].double(), pn, prev[2] + 1e-300, what + " p", report)
            if with_ema:
                KC.check_bound(got[4].double(), en, prev[3] + 1e-300, what + " ema", report)
                Em = en.float()
            else:
                assert torch.equal(got[4], p0), what + ": ema = NULL, but the buffer moved"
            assert torch.equal(got[1], gn.float()), what + ": gradient after the step"
            z = g == 0
            if step == 0 and bool(z.any()) and (decoupled or wd == 0.0):  # m = v = 0, denom = eps: finite, and the decay alone moves p
                want = P.double() * ((1.0 - LRS[0] * wd) if decoupled else 1.0)
                assert bool(((got[0].double() - want).abs() <= 2 * AR.U24 * want.abs())[z].all()), what + ": a zero gradient moved p"
                assert bool((got[2][z] == 0).all()) and bool((got[3][z] == 0).all())
            P, M, V = pn.float(), mn.float(), vn.float()
            prev = AR.carry(prev, outs, has_ema=with_ema)

        for step in range(3):
            g = _gradient(n, gen, step, scale)
            ss = TR.sumsq_ref(g)
            assert (math.sqrt(ss) / (scale or 1.0) > MAX_NORM) == (step == 1) or n == 1
            one(step, ss, g)
        if scale is not None:  # overflowing steps from the state the kernel is in, then a finite one
            for bad in (math.inf, math.nan):
                one(2, bad, torch.ones(n) * scale, skipped=True)
            assert t == 3
            g = _gradient(n, gen, 3, scale)
            one(3, TR.sumsq_ref(g), g)
            assert t == 4
    KC.print_report(report, f"adam n{n}", "comparisons")


@KC.stop_after_fault
def test_step_advance_alone_counts_and_skips():
    """upa_adam_step_advance alone: 0 -> 1 -> 2; with a scaler state, inf and NaN leave the count, a finite norm moves it; without one
    (scaler_state = NULL) a non-finite norm still counts, as the update kernel's predicate has it."""
    DEV, L, lib, st = KC.env()
    Td = Guarded(torch.zeros(1, dtype=torch.int32), 3, 2)
    ss = torch.tensor([1.0, math.inf, math.nan], dtype=F64, device=DEV)
    sstate = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=DEV)
    seen = [int(Td.get("advance")[0])]
    for i, sp in ((0, None), (0, None), (1, sstate.data_ptr()), (2, sstate.data_ptr()), (0, sstate.data_ptr()), (1, None)):
        L.check(lib.upa_adam_step_advance(Td.ptr, ss.data_ptr() + 8 * i, sp, st), "adam_step_advance")
        seen.append(int(Td.get("advance")[0]))
    assert seen == [0, 1, 2, 2, 2, 3, 4], seen
    assert torch.equal(sstate.cpu(), torch.tensor([1024.0, 0.0, 0.0, 0.0]))


@KC.stop_after_fault
def test_refusals_write_nothing():
    """n < 0, a NULL p / g / exp_avg / exp_avg_sq / grad_sumsq / step_dev, a beta outside [0, 1) (1, negative, NaN): UPA_EINVAL through
    upa_last_error, every buffer bit-identical; n = 0 is accepted and writes nothing; the unmodified call is accepted."""
    DEV, L, lib, st = KC.env()
    n = 100
    x = torch.arange(n, dtype=F32) / 7 + 0.5
    bufs = [Guarded(x + i) for i in range(5)]
    Td = Guarded(torch.ones(1, dtype=torch.int32), 1, 1)
    ss = torch.tensor([4.0], dtype=F64, device=DEV)
    before = [b.buf.clone() for b in bufs] + [Td.buf.clone(), ss.clone()]

    def call(p=bufs[0].ptr, g=bufs[1].ptr, m=bufs[2].ptr, v=bufs[3].ptr, e=bufs[4].ptr, n=n, s=ss.data_ptr(), b1=B1, b2=B2, t=Td.ptr):
        return lib.upa_adam_ema(p, g, m, v, e, n, s, MAX_NORM, 1e-3, b1, b2, EPS, 5e-4, 1, t, 0.5, None, 1, None, st)

    refused = [call(n=-1), call(p=None), call(g=None), call(m=None), call(v=None), call(s=None), call(t=None), call(b1=1.0), call(b1=-0.5),
               call(b2=1.0), call(b2=1.5), call(b1=NAN), call(b2=NAN), lib.upa_adam_step_advance(None, ss.data_ptr(), None, st),
               lib.upa_adam_step_advance(Td.ptr, None, None, st)]
    assert refused == [UPA_EINVAL] * len(refused), refused
    assert b"adam" in lib.upa_last_error()
    assert call(n=0) == 0
    torch.cuda.synchronize()
    after = [b.buf for b in bufs] + [Td.buf, ss]
    assert all(KC.same_bits(a, b) for a, b in zip(after, before)), "a refused call (or n = 0) wrote a buffer"
    assert call() == 0
    torch.cuda.synchronize()
    assert not KC.same_bits(bufs[0].buf, before[0]) and int(Td.get("accepted")[0]) == 1
