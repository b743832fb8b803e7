"""-m gpu: every whole-block line-buffer / tile kernel (upa_c2f_fused, upa_c2f32_up_fused, upa_c2f16_down_fused, upa_c2f64_fused, the
upa_bottleneck_pair family, upa_detect_level_stream) against the float64 chain reference of tests/block_ref.py, element by element: inside
the reference's bound everywhere and BIT-EQUAL to the reference's bf16 value wherever that bound is 0 (most elements of the `positive`
family).  No term of the bound is tied to the largest output, and none was read off a GPU run.

Buffers, sentinels, the two bit-identical runs, the per-element bounds and the fault latch: the conventions of tests/kernel_check.py
(E = 8, a spare
image behind the output; the virtually upsampled slice of a concat buffer is NaN: never read).  The form under test is asserted to have been
dispatched (`_fused` / `_form32up` / `_form64` / `forward_down` / the C entry point's return code) under the `upa_opts` that select it.

BLOCK_STATS=1 prints, per case, the share of outputs held bit-exact and the worst |kernel - ref| / bound over the other elements."""

import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import block_ref as B
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

E = 8  # spare channels on either side of a slice (16 bytes: the kernels' alignment)
NAN = float("nan")
PARAMS = [pytest.param(i, fam, id=f"{c['id']}-{fam}") for i, c in enumerate(B.CASES) for fam in B.FAMILIES]


def _dev_slice(x_nchw, lead_nan=0):
    """CPU NCHW float32 (bf16-exact) -> a device NHWC channel slice [E, E + c) of a NaN-filled buffer; its first `lead_nan` channels NaN too."""
    buf = KC.slice_buf(x_nchw.permute(0, 2, 3, 1), torch.bfloat16, E, lead_fill=lead_nan)
    return buf.permute(0, 3, 1, 2)[:, E:E + x_nchw.shape[1]]


def _out_view(n, c, h, w):
    buf = KC.out_buf((n, h, w), c + 2 * E, torch.bfloat16, 1)
    return buf, buf.permute(0, 3, 1, 2)[:n, E:E + c]


def _opts(case):
    """The case's `upa_opts` switches on top of the session's options (no switch: the options in force, untouched)."""
    from ultralytics_pro_amd.engine import runtime as R
    return R.use_opts(**case["opts"]) if case["opts"] else contextlib.nullcontext()


def _load(conv, wb):
    """Put (w, bias) into a Conv module so that BN folding returns exactly them: gamma 1, mean 0, var 1, eps 0, beta = bias."""
    w, b = wb
    assert tuple(conv.conv.weight.shape) == tuple(w.shape), (conv.conv.weight.shape, w.shape)
    conv.conv.weight.data = w.clone()
    conv.bn.weight.data.fill_(1.0)
    conv.bn.bias.data = b.clone()
    conv.bn.running_mean.zero_()
    conv.bn.running_var.fill_(1.0)
    conv.bn.eps = 0.0


def _c2f_module(case, wts):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.nn import modules as pm
    c1 = case.get("c1", 64)
    m = pm.C2f(c1, case.get("c2", 64), case.get("nb", 1), case["sc"]).eval()
    assert m.c == case.get("c", 32)
    _load(m.cv1, wts["cv1"])
    _load(m.cv2, wts["cv2"])
    for bt, (a, b) in zip(m.m, wts["m"]):
        _load(bt.cv1, a)
        _load(bt.cv2, b)
    return m.to(DEV)


def _run_block(case, d):
    """Launch the case's kernel once into fresh poisoned buffers -> (whole output buffer on the CPU as float32 NHWC, slice bounds)."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn import modules as pm
    from ultralytics_pro_amd.nn.modules.conv import PackedConv, VirtualUpsample
    form, n, h, w = case["form"], case["n"], case["h"], case["w"]
    with torch.no_grad(), _opts(case):
        if form in ("c2f", "c2f_down"):
            m = _c2f_module(case, d["wts"])
            m.fuse_block = True
            upc = case.get("upc", 0)
            xd = _dev_slice(d["x"], lead_nan=upc)
            up, mat = None, []
            if upc:
                ud = _dev_slice(d["u"])
                up = VirtualUpsample(ud, upc, lambda: mat.append(1))
            if form == "c2f_down":
                md = pm.Conv(32, 64, 3, 2).eval()
                _load(md, d["wts"]["down"])
                md = md.to(DEV)
                buf, out = _out_view(n, 64, (h + 1) // 2, (w + 1) // 2)
                y = m.forward_down(xd, md, out=out)
                assert y is not None, "upa_c2f16_down_fused was not dispatched"
            else:
                if case["c"] == 64:
                    assert m._form64()
                elif case["c1"] >= 128:
                    assert m._form32up()
                buf, out = _out_view(n, case["c2"], h, w)
                y = m._fused(xd, out, up)
                assert y is not None, "the fused form was not dispatched"
                assert not mat and (up is None or not up.done), "the fused block must read the half-resolution tensor itself"
            c_out = out.shape[1]
        elif form in ("pair", "pair_e"):
            c, cm = case["c"], case["cm"]
            (wa, ba), (wb, bb) = d["wts"]
            p1, p2 = PackedConv(wa, ba, 3, DEV, torch.bfloat16, False), PackedConv(wb, bb, 3, DEV, torch.bfloat16, False)
            xd = _dev_slice(d["x"])
            buf, out = _out_view(n, c, h, w)
            vx, vy = R.view_of(xd), R.view_of(out)
            if form == "pair":
                rc = L.lib().upa_bottleneck_pair(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, p1.w.data_ptr(), p1.bias.data_ptr(), p2.w.data_ptr(),
                                                 p2.bias.data_ptr(), vy.ptr, vy.ld, int(case["sc"]), L.ACT_SILU, vx.dtype, R.opts_ptr(), L.current_stream(DEV))
            else:
                rc = L.lib().upa_bottleneck_pair_e(vx.ptr, vx.n, vx.h, vx.w, vx.c, cm, vx.ld, p1.w.data_ptr(), p1.bias.data_ptr(), p2.w.data_ptr(),
                                                   p2.bias.data_ptr(), vy.ptr, vy.ld, int(case["sc"]), L.ACT_SILU, vx.dtype, R.opts_ptr(), L.current_stream(DEV))
            assert rc != L.UPA_EUNSUPPORTED, "the pair kernel must be dispatched under the test options (pair = 2)"
            L.check(rc, form)
            c_out = c
        else:
            assert form == "pair_cv2", form
            m = _c2f_module(dict(case, c1=64, c2=64, nb=1, c=32), d["wts"])
            cat = _dev_slice(torch.cat([d["x"], torch.zeros(n, 32, h, w)], 1), lead_nan=0)  # [y0 | y1 | room for b] as C2f lays it out
            cat[:, 64:].fill_(NAN)  # the fused launch never writes or reads b
            buf, out = _out_view(n, 64, h, w)
            assert m._pair_cv2(cat, out) is not None, "upa_bottleneck_pair_cv2 was not dispatched"
            c_out = 64
    torch.cuda.synchronize()
    return buf.cpu(), c_out


def _report(stats, case, fam):
    if os.environ.get("BLOCK_STATS"):
        for what, z, s in stats:
            print(f"BLOCK_STATS {case['kernel']}|{case['id']}|{fam}|{what}|exact={z:.4f}|worst_share={s:.4f}", flush=True)


@pytest.mark.parametrize("ci,fam", [p for p in PARAMS if B.CASES[p.values[0]]["form"] != "detect"])
@KC.stop_after_fault
def test_block_kernel_vs_f64_chain(ci, fam):
    case = B.CASES[ci]
    d, (ref, e) = B.reference(ci, fam)
    n = case["n"]
    buf, c_out = KC.twice(lambda: _run_block(case, d))
    got = KC.payload(buf, n, c_out, "out", offset=E).permute(0, 3, 1, 2).to(torch.float64)
    share = KC.check_bound(got, ref, e, "out", exact_where_zero=True)
    stats = [("out", float((e == 0).float().mean()), share)]
    _report(stats, case, fam)


def _run_detect(case, d):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    n, h, w, nc = case["n"], case["h"], case["w"], case["nc"]
    a0, extra = 19, 5
    a_total = a0 + h * w + extra
    y = torch.full((n + 1, 4 + nc, a_total), NAN, device=DEV)
    keys = torch.full((n + 1, a_total), -1, dtype=torch.int64, device=DEV)
    xd = _dev_slice(d["x"])
    vx = R.view_of(xd)
    branches, keep = [], []
    for name, c, cout, ct in (("box", 64, 64, 64), ("cls", 80, nc, 80)):
        (w1, b1), (w2, b2), (wt, bt) = d["wts"][name]
        wtp = torch.cat([wt, torch.zeros(ct - cout, c, 1, 1)], 0)
        btp = torch.cat([bt, torch.zeros(ct - cout)], 0)
        pk = [PackedConv(w1, b1, 3, DEV, torch.bfloat16, False), PackedConv(w2, b2, 3, DEV, torch.bfloat16, False),
              PackedConv(wtp, btp, 1, DEV, torch.bfloat16, False)]
        keep += pk
        branches.append(L.DetectBranch(c, 0, pk[0].w.data_ptr(), pk[0].bias.data_ptr(), pk[1].w.data_ptr(), pk[1].bias.data_ptr(), pk[2].w.data_ptr(),
                                       pk[2].bias.data_ptr()))
    with _opts(case):
        rc = L.lib().upa_detect_level_stream(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, C.byref(branches[0]), C.byref(branches[1]), nc, 8.0,
                                             y.data_ptr(), a_total, a0, keys.data_ptr(), L.UPA_BF16, R.opts_ptr(), L.current_stream(DEV))
    assert rc != L.UPA_EUNSUPPORTED, "upa_detect_level_stream refused the level"
    L.check(rc, "detect_level_stream")
    torch.cuda.synchronize()
    return y.cpu(), keys.cpu(), a0


TWINS_PARAMS = [pytest.param(i, "twins", id=f"{B.CASES[i]['id']}-twins") for i in B.TWINS_CASES]


@pytest.mark.parametrize("ci,fam", [p for p in PARAMS if B.CASES[p.values[0]]["form"] == "detect"] + TWINS_PARAMS)
@KC.stop_after_fault
def test_detect_level_stream_vs_f64_chain(ci, fam):
    case = B.CASES[ci]
    d, (bl, be, cl, ce, _) = B.reference(ci, fam)
    n, h, w, nc = case["n"], case["h"], case["w"], case["nc"]
    keys_only = case["opts"]["keys_only"]
    dec = B.detect_decode(bl, be, cl, ce, 8.0)
    y, keys, a0 = KC.twice(lambda: _run_detect(case, d))
    hw = h * w
    lvl = slice(a0, a0 + hw)
    assert bool(torch.isnan(y[n]).all()) and bool(torch.isnan(y[:, :, :a0]).all()) and bool(torch.isnan(y[:, :, a0 + hw:]).all()), "wrote outside the level"
    assert bool((keys[n] == -1).all()) and bool((keys[:, :a0] == -1).all()) and bool((keys[:, a0 + hw:] == -1).all())
    stats = []
    got = y[:n, :, lvl].to(torch.float64)

    def inside(g, r, e, what):
        stats.append((what, float((e == 0).float().mean()), KC.check_bound(g, r, e, what)))
    inside(got[:, :4], dec["box"], dec["e_box"], "box")
    kbits = keys[:n, lvl].numpy().view(np.uint64)
    kscore = torch.from_numpy((~(kbits >> np.uint64(32)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32))
    kidx = (kbits & np.uint64(0xFFFFFFFF)).astype(np.int64)
    kcls = torch.from_numpy(kidx - np.arange(a0, a0 + hw, dtype=np.int64)[None, :] * nc)
    assert bool(((kcls >= 0) & (kcls < nc)).all())
    sref, es = dec["score"], dec["e_score"]
    if keys_only:
        assert bool(torch.isnan(y[:n, 4:, lvl]).all()), "keys-only: the class rows must stay untouched"
    else:
        inside(got[:, 4:], sref, es, "score")
        # the keys are exactly the first maxima of the scores the kernel itself wrote (utils/nms key order, nms.py:109)
        best, arg = y[:n, 4:, lvl].max(1)
        assert torch.equal(kscore, best) and torch.equal(kcls, arg)
    # the key's score is the score of the class it names, within that class's bound
    ks_ref = sref.gather(1, kcls.unsqueeze(1)).squeeze(1)
    ks_e = es.gather(1, kcls.unsqueeze(1)).squeeze(1)
    inside(kscore.to(torch.float64), ks_ref, ks_e, "key score")
    # ... and its class is the reference's argmax wherever the reference's top-two margin exceeds the sum of the two score bounds
    top, idx = sref.topk(2, dim=1)
    clear = (top[:, 0] - top[:, 1]) > es.gather(1, idx).sum(1)
    assert bool((kcls == idx[:, 0])[clear].all()), "best class differs where the reference decides it"
    stats.append(("key class decided", float(clear.float().mean()), 0.0))
    if fam == "twins":
        # ties made by construction (block_ref.TWIN_GROUPS / TWIN_SAT): the first index of identical rows, the larger bias of a 2^-14 /
        # 2^-13 pair, the first of the rows that all score 1.0f
        want, decided = B.twins_answer(cl, ce)
        assert bool(decided[:, :3].all()) and bool((want == B.TWIN_SAT[0])[:, :3].all())  # (the dark columns: anchors 0..2 of row 0)
        assert bool((kcls == want)[decided].all()), "best class differs from the constructed answer"
        stats.append(("key class constructed", float(decided.float().mean()), 0.0))
    _report(stats, case, fam)
