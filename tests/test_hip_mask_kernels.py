"""-m gpu: the mask kernels of csrc/segment.hip through the C ABI, held to tests/mask_ref.py (pinned on the CPU by
tests/test_mask_ref.py) under the conventions of tests/kernel_check.py: `upa_process_mask` on every tile form, depth, store path,
the row loop's second trip, 1024 images and a mode-0 window offset, with proto channel slices between NaN neighbours, two row
layouts, guard rows behind the capacity and two runs compared byte for byte; its refusals; `upa_mask_coef_rows`,
`upa_nms_gather_extra`, `upa_resize_bilinear`, `upa_crop_mask` and `upa_copy_rows`, each once past its grid cap.

`upa_process_mask` per case on one MI355X (undecided pixels / of them unlike the reference's v > 0): see DESIGN.md section 2."""

import numpy as np
import pytest
import torch

from tests import kernel_check as KC
from tests import mask_ref as R

pytestmark = pytest.mark.gpu
NAN = KC.NAN
_T = {"f32": torch.float32, "bf16": torch.bfloat16}
RUN = [(c, d) for c in R.mask_kernel_cases() if not getattr(c, "refused", False) for d in c.dtypes]


def _code(L, dtype):
    return L.UPA_F32 if dtype == "f32" else L.UPA_BF16


def _err(lib):
    return lib.upa_last_error().decode(errors="replace")


# ---- upa_process_mask ---------------------------------------------------------------------------------------------------------------
def _row_buffers(case, inp, dev):
    """The coefficients and boxes twice: as columns of one (b, max_det, 6 + nm + 3) row buffer (coef_ld == det_ld), and as two
    buffers of their own pitches.  Rows past the counts, and every other column, are NaN."""
    b, md, nm = case.b, case.max_det, case.nm
    rows = torch.full((b, md, 6 + nm + 3), NAN)
    coef = torch.full((b, md, nm + 5), NAN)
    det = torch.full((b, md, 7), NAN)
    for i, n in enumerate(case.counts):
        rows[i, :n, :4], rows[i, :n, 4], rows[i, :n, 5] = inp.boxes[i, :n], 0.5, 0.0
        rows[i, :n, 6:6 + nm] = inp.coef[i, :n]
        coef[i, :n, :nm] = inp.coef[i, :n]
        det[i, :n, :4] = inp.boxes[i, :n]
    rows, coef, det = rows.to(dev), coef.to(dev), det.to(dev)
    return {"rows": (rows, rows.data_ptr() + 24, 6 + nm + 3, rows.data_ptr(), 6 + nm + 3),
            "split": (None, coef.data_ptr(), nm + 5, det.data_ptr(), 7), "_keep": (rows, coef, det)}


@pytest.mark.parametrize("case,dtype", RUN, ids=[f"{c.name}-{d}" for c, d in RUN])
@KC.stop_after_fault
def test_process_mask(case, dtype):
    DEV, L, lib, stream = KC.env()
    inp, ref = R.case_reference(case, dtype)
    tdt = _T[dtype]
    E = 16 // torch.empty((), dtype=tdt).element_size()
    nm, (mh, mw), (H, W) = case.nm, case.mhw, case.out_hw
    pbuf = KC.slice_buf(inp.protos, tdt, E)  # (b, mh, mw, E + nm + E), NaN beside the slice
    pptr, ldp = pbuf.data_ptr() + 16, nm + 2 * E
    bufs = _row_buffers(case, inp, DEV)
    cnt = torch.tensor(case.counts, dtype=torch.int32, device=DEV)
    total_rows = sum(case.counts)
    top, left, bottom, right = case.window
    assert R.tile_form((bottom - top, right - left), (H, W)) is not None

    def run(layout, cap):
        _, cptr, cld, dptr, dld = bufs[layout]
        masks = torch.full((cap + 3, H, W), 7, dtype=torch.uint8, device=DEV)
        flags = torch.full((cap + 3,), 5, dtype=torch.int32, device=DEV)
        total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        L.check(lib.upa_process_mask(pptr, case.b, mh, mw, nm, ldp, _code(L, dtype), cptr, cld, dptr, dld, case.max_det, cnt.data_ptr(), H, W,
                                     case.mode, float(case.ratio[0]), float(case.ratio[1]), top, left, bottom, right, masks.data_ptr(),
                                     flags.data_ptr(), cap, total.data_ptr(), stream), "process_mask")
        torch.cuda.synchronize()
        return masks, flags, total

    for cap in case.capacities:
        what = f"{case.name} {dtype} capacity {cap}"
        first, again, split = run("rows", cap), run("rows", cap), run("split", cap)
        for k, name in enumerate(("masks", "nonempty", "total")):
            assert KC.same_bits(first[k], again[k]), f"{what}: two runs differ in {name}"
            assert KC.same_bits(first[k], split[k]), f"{what}: the two row layouts differ in {name}"
        m, flags, total = first[0].cpu().numpy(), first[1].cpu().numpy(), int(first[2].item())
        n = min(total_rows, cap)
        assert total == total_rows, f"{what}: total {total}, counts sum to {total_rows}"
        assert (m[n:] == 7).all(), f"{what}: mask rows past the written ones touched"
        assert (flags[cap:] == 5).all() and (flags[n:cap] == 0).all(), f"{what}: nonempty past the written rows"
        m = m[:n]
        assert (m <= 1).all(), f"{what}: a mask byte is neither 0 nor 1"
        got = m == 1
        dec, bit = ref.decided[:n], ref.bit[:n]
        bad = (got != bit) & dec
        assert not bad.any(), (f"{what}: {int(bad.sum())} decided pixels differ from the reference (first at "
                               f"{tuple(int(v) for v in np.argwhere(bad)[0])}: v = {ref.v[:n][bad][0]!r}, bound {ref.bound[:n][bad][0]!r})")
        anyrow = got.reshape(n, -1).any(1)
        assert np.array_equal(flags[:n], anyrow.astype(np.int32)), f"{what}: nonempty is not any(bits) of its row"
        assert flags[:n][(dec & bit).reshape(n, -1).any(1)].all(), f"{what}: nonempty 0 on a row with a decided set pixel"
        und = ~dec
        print(f"{what}: {int(und.sum())} undecided of {int(ref.inside[:n].sum())} inside pixels, "
              f"{int((got != (ref.inside[:n] & (ref.v[:n] > 0)))[und].sum())} of them unlike v > 0")
    assert bool(torch.isnan(pbuf[..., :E].float()).all()) and bool(torch.isnan(pbuf[..., E + nm:].float()).all())


@KC.stop_after_fault
def test_process_mask_refusals_write_nothing():
    DEV, L, lib, stream = KC.env()
    refused = [c for c in R.mask_kernel_cases() if getattr(c, "refused", False)][0]
    assert R.tile_form(refused.mhw, refused.out_hw) is None

    def call(why, rc_want, b=1, mhw=(4, 4), nm=8, dtype="f32", mode=0, out_hw=(8, 8), window=None, cap=2, null_masks=False, ldp=None):
        mh, mw = mhw
        tdt = _T[dtype]
        p = torch.zeros((b, mh, mw, ldp or nm), dtype=tdt, device=DEV)
        rows = torch.zeros((b, 2, 6 + nm), device=DEV)
        cnt = torch.ones((b,), dtype=torch.int32, device=DEV)
        masks = torch.full((max(cap, 1) + 1, *out_hw), 7, dtype=torch.uint8, device=DEV)
        flags = torch.full((max(cap, 1) + 1,), 5, dtype=torch.int32, device=DEV)
        total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        top, left, bottom, right = window or (0, 0, mh, mw)
        rc = lib.upa_process_mask(p.data_ptr(), b, mh, mw, nm, ldp or nm, _code(L, dtype), rows.data_ptr() + 24, 6 + nm, rows.data_ptr(), 6 + nm, 2,
                                  cnt.data_ptr(), out_hw[0], out_hw[1], mode, 1.0, 1.0, top, left, bottom, right,
                                  None if null_masks else masks.data_ptr(), None if null_masks else flags.data_ptr(), cap, total.data_ptr(),
                                  stream)
        torch.cuda.synchronize()
        if rc_want == 0:
            assert rc == 0, (why, _err(lib))
            return masks, flags, total
        assert rc == rc_want and why in _err(lib), (rc, _err(lib))
        assert bool((masks == 7).all()) and bool((flags == 5).all()) and int(total.item()) == -1, f"{why}: a refused call wrote"

    call("does not fit the tile buffer", L.UPA_EUNSUPPORTED, mhw=refused.mhw, out_hw=refused.out_hw, mode=1)
    call("nm 136", L.UPA_EUNSUPPORTED, nm=136)
    call("16-byte groups", L.UPA_EINVAL, nm=12, dtype="bf16", ldp=16)
    call("b 1025", L.UPA_EUNSUPPORTED, b=R.PM_B + 1, mhw=(2, 2), out_hw=(2, 2))
    call("mode 2", L.UPA_EUNSUPPORTED, mode=2)
    call("bad source window", L.UPA_EINVAL, window=(0, 0, 5, 4))
    call("bad shape", L.UPA_EINVAL, null_masks=True)
    masks, flags, total = call("capacity 0", 0, b=3, cap=0, null_masks=True)
    assert int(total.item()) == 3 and bool((masks == 7).all()) and bool((flags == 5).all())


# ---- upa_mask_coef_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 32, 5, 7, 3, 13), (3, 32, 160, 160, 3, 16)], ids=["5x7", "grid_cap"])
@KC.stop_after_fault
def test_mask_coef_rows(shape, dtype):
    """NHWC level map -> (n, c_total, a_total) rows at (c0, a0): exact (bf16 -> f32 widens exactly), all else still NaN.
    grid_cap: 3 * 32 * 160 * 160 elements > 8192 workgroups * 256, the stride loop's second trip."""
    DEV, L, lib, stream = KC.env()
    n, c, h, w, c0, a0 = shape
    tdt = _T[dtype]
    E = 16 // torch.empty((), dtype=tdt).element_size()
    x = KC.unit_input(f"maskk:coefrows:{shape}", (n, h, w, c)).to(tdt).float()
    xbuf = KC.slice_buf(x, tdt, E)
    c_total, a_total = c0 + c + 2, a0 + h * w + 5
    es = xbuf.element_size()

    def run():
        out = torch.full((n + 1, c_total, a_total), NAN, device=DEV)
        L.check(lib.upa_mask_coef_rows(xbuf.data_ptr() + E * es, n, h, w, c, c + 2 * E, _code(L, dtype), out.data_ptr(), c_total, c0, a_total, a0,
                                       stream), "mask_coef_rows")
        torch.cuda.synchronize()
        return out

    out = KC.twice(run).cpu()
    want = torch.full((n + 1, c_total, a_total), NAN)
    want[:n, c0:c0 + c, a0:a0 + h * w] = x.reshape(n, h * w, c).permute(0, 2, 1)
    assert KC.same_bits(out, want)
    if h * w < 100:
        keep = torch.full((n, c_total, a_total), NAN, device=DEV)
        for why, kw in (("c0 + c > c_total", dict(c_total=c0 + c - 1)), ("a0 + hw > a_total", dict(a_total=a0 + h * w - 1)), ("ldx < c", dict(ldx=c - 4))):
            a = dict(c_total=c_total, a_total=a_total, ldx=c + 2 * E)
            a.update(kw)
            rc = lib.upa_mask_coef_rows(xbuf.data_ptr() + E * es, n, h, w, c, a["ldx"], _code(L, dtype), keep.data_ptr(), a["c_total"], c0,
                                        a["a_total"], a0, stream)
            torch.cuda.synchronize()
            assert rc == L.UPA_EINVAL and "mask_coef_rows: bad shape" in _err(lib), why
            assert bool(torch.isnan(keep).all()), why


# ---- upa_nms_gather_extra -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_det", [True, False], ids=["det", "no_det"])
@pytest.mark.parametrize("shape", [(3, 7, 5, 11, (7, 0, 3)), (32, 300, 128, 64, None)], ids=["small", "grid_cap"])
@KC.stop_after_fault
def test_nms_gather_extra(shape, with_det):
    """grid_cap: 32 * 300 * (128 | 134) elements > 4096 workgroups * 256."""
    DEV, L, lib, stream = KC.env()
    b, md, ne, a, counts = shape
    counts = list(counts) if counts else [(37 * i) % (md + 1) for i in range(b - 1)] + [md]
    extra = KC.unit_input(f"maskk:gather:{shape}", (b, ne, a))
    keep = (KC.unit_input(f"maskk:gather:k:{shape}", (b, md), 0.0, float(a)).floor().clamp(0, a - 1)).to(torch.int32)
    keep[0, 0], keep[0, 1], keep[0, 2] = -1, a, a + 5  # outside [0, a): exact zeros
    det = torch.full((b, md, 6), NAN)
    for i, n in enumerate(counts):
        keep[i, n:] = 10 ** 6  # rows past the counts are not looked up
        det[i, :n] = KC.unit_input(f"maskk:gather:d:{shape}:{i}", (n, 6), 0.0, 100.0)
    cols = ne + (6 if with_det else 0)
    ldo = cols + 3
    want = torch.full((b * md + 2, ldo), NAN)
    body = torch.zeros((b, md, cols))
    for i, n in enumerate(counts):
        k = keep[i, :n].long()
        ok = (k >= 0) & (k < a)
        g = extra[i][:, k.clamp(0, a - 1)].t() * ok[:, None]
        body[i, :n, cols - ne:] = torch.where(ok[:, None], g, torch.zeros_like(g))
        if with_det:
            body[i, :n, :6] = det[i, :n]
    want[:b * md, :cols] = body.reshape(b * md, cols)
    ed, kd, dd = extra.to(DEV), keep.to(DEV), det.to(DEV)
    cd = torch.tensor(counts, dtype=torch.int32, device=DEV)

    def run():
        out = torch.full((b * md + 2, ldo), NAN, device=DEV)
        L.check(lib.upa_nms_gather_extra(ed.data_ptr(), b, ne, a, kd.data_ptr(), cd.data_ptr(), md, dd.data_ptr() if with_det else None,
                                         out.data_ptr(), ldo, stream), "nms_gather_extra")
        torch.cuda.synchronize()
        return out

    assert KC.same_bits(KC.twice(run), want)


# ---- upa_resize_bilinear ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.resize_cases(), ids=lambda c: c[0])
@KC.stop_after_fault
def test_resize_bilinear(case):
    """Inside resize_reference's derived bound; the source outside the window is NaN, the output lies in a NaN buffer with two
    spare planes."""
    DEV, L, lib, stream = KC.env()
    name, planes, (h, w), window, (oh, ow) = case
    top, left, bottom, right = window
    x = R.resize_input(name, planes, (h, w))
    v, bound = R.resize_reference(x.numpy(), window, (oh, ow))
    xin = torch.full((planes, h, w), NAN)
    xin[:, top:bottom, left:right] = x[:, top:bottom, left:right]
    xd = xin.to(DEV)

    def run(p=planes):
        out = torch.full((planes + 2, oh, ow), NAN, device=DEV)
        L.check(lib.upa_resize_bilinear(xd.data_ptr(), p, h, w, top, left, bottom, right, out.data_ptr(), oh, ow, stream), "resize_bilinear")
        torch.cuda.synchronize()
        return out

    out = KC.twice(run).cpu()
    assert bool(torch.isnan(out[planes:]).all()), "wrote past the last plane"
    share = KC.check_bound(out[:planes].double(), v, bound, f"resize {name}")
    print(f"resize {name}: worst error / bound = {share:.3f}")
    assert bool(torch.isnan(run(0)).all()), "planes = 0 wrote"


# ---- upa_crop_mask ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 24, 36), (9, 512, 512)], ids=["24x36", "grid_cap"])
@KC.stop_after_fault
def test_crop_mask(shape):
    """`masks * bool` with box_ld = 7: the bits of m * float(inside) computed on the CPU, -0.0 and the zero a negative value leaves
    included; NaN stays NaN inside and outside the box (its payload is not compared)."""
    from tests.test_hip_segval import _boxes
    DEV, L, lib, stream = KC.env()
    n, h, w = shape
    m = KC.unit_input(f"maskk:crop:{shape}", (n, h, w))
    u = KC.unit_input(f"maskk:crop:u:{shape}", (n, h, w), 0.0, 1.0)
    m[u < 0.05] = -0.0
    m[u > 0.95] = NAN
    boxes = torch.full((n, 7), NAN)
    boxes[:, :4] = torch.from_numpy(_boxes(n, h, w, f"maskk:crop:b:{shape}"))
    inside = torch.from_numpy(R.in_box(np.arange(w), np.arange(h), boxes[:, :4].numpy()))
    want = m * inside.float()
    assert bool(inside.any()) and not bool(inside.all())
    md, bd = m.to(DEV), boxes.to(DEV)

    def run():
        out = torch.full((n + 1, h, w), NAN, device=DEV)
        L.check(lib.upa_crop_mask(md.data_ptr(), n, h, w, bd.data_ptr(), 7, out.data_ptr(), stream), "crop_mask")
        torch.cuda.synchronize()
        return out

    out = KC.twice(run).cpu()
    assert bool(torch.isnan(out[n:]).all()), "wrote past the last plane"
    got, nan = out[:n], torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(KC.bits(got)[~nan], KC.bits(want)[~nan])
    assert bool((KC.bits(want)[~nan] == KC.bits(torch.tensor([-0.0]))[0]).any())


# ---- upa_copy_rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(13, 5, 9, 7), (70000, 31, 33, 36)], ids=["13x5", "grid_cap"])
@KC.stop_after_fault
def test_copy_rows(shape):
    DEV, L, lib, stream = KC.env()
    rows, cols, lds, ldd = shape
    src = torch.full((rows, lds), NAN)
    src[:, :cols] = KC.unit_input(f"maskk:copy:{shape}", (rows, cols))
    sd = src.to(DEV)
    want = torch.full((rows + 2, ldd), NAN)
    want[:rows, :cols] = src[:, :cols]

    def run(r=rows, c=cols):
        dst = torch.full((rows + 2, ldd), NAN, device=DEV)
        L.check(lib.upa_copy_rows(sd.data_ptr(), r, c, lds, dst.data_ptr(), ldd, stream), "copy_rows")
        torch.cuda.synchronize()
        return dst

    assert KC.same_bits(KC.twice(run), want)
    assert bool(torch.isnan(run(0, cols)).all()) and bool(torch.isnan(run(rows, 0)).all())
