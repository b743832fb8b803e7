"""-m gpu: segmentation validation on the HIP path (csrc/segval.hip): ground-truth packing (`upa_pack_mask_bits`), the fused mask
matching (`upa_segment_match`: its mask bits against `upa_process_mask`, its IoU and true positives against the integer checker
tests/segval_ref.py and the reference goldens), `mask_iou`, the refusals, SegmentationValidator end to end and under graph replay.

House convention: every output buffer is filled with 0xFF / NaN sentinels first, every kernel result is taken twice and compared
bit for bit."""

import numpy as np
import pytest
import torch

from tests import segval_ref as V
from tests import kernel_check as KC
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def OPS(golden_dir):
    return np.load(golden_dir / "ops_segval.npz")


@pytest.fixture(scope="module")
def MAP(golden_dir):
    return np.load(golden_dir / "map_yolov8n-seg.npz")


def _dev():
    from tests.hip_utils import DEV
    return DEV


def _i32(a):
    """uint32 words -> the int32 tensor the wrappers carry them in."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. packing -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hw", [(8, 8), (20, 28), (160, 160)])
@KC.stop_after_fault
def test_pack_mask_bits(hw):
    from ultralytics_pro_amd.utils import metrics as M
    dev = _dev()
    h, w = hw
    npix, words = h * w, V.words_of(h * w)
    ngt = [0, 1, 5]
    b, max_gt = 3, 6
    # index maps: label k of image i covers a hash-chosen band; later labels overwrite earlier ones as Format's overlap masks do
    idx = np.zeros((b, h, w), np.int64)
    for i, n in enumerate(ngt):
        u = P.hash_uniform(f"segval:pack:{hw}:{i}", 4 * max(n, 1)).reshape(-1, 4)
        for k in range(n):
            y0, x0 = int(u[k, 0] * (h - 2)), int(u[k, 1] * (w - 2))
            idx[i, y0:y0 + 2 + int(u[k, 2] * h / 2), x0:x0 + 2 + int(u[k, 3] * w / 2)] = k + 1
    idx[1, 0, 0] = 7  # an index past ngt[1] = 1 belongs to no label
    want = np.zeros((b, max_gt, npix), bool)
    for i, n in enumerate(ngt):
        for k in range(n):
            want[i, k] = (idx[i] == k + 1).reshape(-1)
    want_bits, want_area = V.pack_bits(want.reshape(b * max_gt, npix)).reshape(b, max_gt, words), want.sum(-1).astype(np.int32)
    assert want_area[2].min() >= 0 and want_area[2].max() > 0
    planes = np.concatenate([want[i, :n].reshape(n, h, w) for i, n in enumerate(ngt)], 0)  # ragged per-instance form: 6 planes
    ngt_d = torch.tensor(ngt, dtype=torch.int32, device=dev)

    def run(src, overlap):
        def once():
            bits, area = M.pack_mask_bits(src, b, max_gt, ngt_d, overlap=overlap)
            return bits.clone(), area.clone()
        # sentinels: the allocator hands the freed block back, so fill one of the same size first
        torch.full((b, max_gt, words), -1, dtype=torch.int32, device=dev)
        bits, area = KC.twice(once)
        assert np.array_equal(_u32(bits), want_bits), (hw, src.dtype, overlap)
        assert np.array_equal(area.cpu().numpy(), want_area)

    for dt in (torch.uint8, torch.int32, torch.float32):
        run(torch.from_numpy(idx).to(dt).to(dev), True)
    for dt in (torch.uint8, torch.float32):
        src = torch.from_numpy(planes.astype(np.float32))
        if dt == torch.float32:
            src = src * 0.75 + 0.125  # 0.125 / 0.875: the threshold is 0.5, not 0
        run(src.to(dt).to(dev), False)
    # sentinel check proper: pre-filled outputs through the C entry
    from ultralytics_pro_amd import _lib as L
    bits = torch.full((b, max_gt, words), -1, dtype=torch.int32, device=dev)
    area = torch.full((b, max_gt), -1, dtype=torch.int32, device=dev)
    src = torch.from_numpy(idx).to(torch.int32).to(dev)
    L.check(L.lib().upa_pack_mask_bits(src.data_ptr(), L.MASK_I32, L.MASKS_OVERLAP, b, b, max_gt, h, w, ngt_d.data_ptr(), bits.data_ptr(),
                                       area.data_ptr(), L.current_stream(dev)))
    torch.cuda.synchronize()
    assert np.array_equal(_u32(bits), want_bits) and np.array_equal(area.cpu().numpy(), want_area)
    assert not _u32(bits)[0].any() and not _u32(bits)[1, 1:].any()  # rows >= ngt
    if npix % 32:
        assert not (_u32(bits)[..., -1] >> (npix % 32)).any()  # padding bits


@KC.stop_after_fault
def test_pack_masks_resizes_like_the_reference():
    """SegmentationValidator.pack_masks on 320 x 320 label masks (overlap form and planes) for a 160 x 160 proto map equals
    F.interpolate(bilinear, align_corners = False) > 0.5 on the CPU (segment/val.py:138-141)."""
    from ultralytics_pro_amd.engine.validator import SegmentationValidator
    dev = _dev()
    n = [2, 0, 3]
    # A 2 x downsample averages 2 x 2 source blocks, so a free-form mask has interpolated values of exactly 0.5 along its edges,
    # where > 0.5 is decided by the last bit.  The source here has none: ellipses drawn at 160 x 160 and doubled (blocks of 0 or 4
    # set pixels), then one hash-chosen pixel cleared in a tenth of the label blocks (3 of 4: 0.75) and one set to label 1 in a tenth
    # of the background blocks (1 of 4: 0.25).
    yy, xx = np.mgrid[0:160, 0:160]
    idx = np.zeros((3, 320, 320), np.uint8)
    for i, k in enumerate(n):
        small = np.zeros((160, 160), np.uint8)
        u = P.hash_uniform(f"segval:resize:{i}", 4 * max(k, 1)).reshape(-1, 4)
        for j in range(k):
            small[((yy - 20 - 120 * u[j, 0]) / (12 + 30 * u[j, 2])) ** 2 + ((xx - 20 - 120 * u[j, 1]) / (12 + 30 * u[j, 3])) ** 2 <= 1] = j + 1
        big = np.kron(small, np.ones((2, 2), np.uint8))
        f = P.hash_uniform(f"segval:resize:flip:{i}", 2 * 160 * 160).reshape(2, 160, 160)
        by, bx = np.nonzero(f[0] < 0.1)
        py, px = 2 * by + (f[1, by, bx] < 0.5), 2 * bx + ((f[1, by, bx] * 4).astype(int) % 2)
        big[py, px] = np.where(small[by, bx] > 0, 0, 1 if k else 0)
        idx[i] = big
    planes = []
    for i, k in enumerate(n):
        planes += [(idx[i] == j + 1) for j in range(k)]
    planes = torch.from_numpy(np.stack(planes)).float()
    val = torch.nn.functional.interpolate(planes[None], (160, 160), mode="bilinear", align_corners=False)[0]
    assert int(((val - 0.5).abs() <= 1e-6).sum()) == 0  # no pixel on the threshold: the comparison below is exact
    assert bool((val == 0.25).any()) and bool((val == 0.75).any())  # ... and not a plain pixel pick either
    want = (val > 0.5).numpy()
    labels = dict(batch_idx=torch.tensor([0, 0, 2, 2, 2]), cls=torch.zeros(5), bboxes=torch.zeros(5, 4))
    for overlap, masks in ((True, torch.from_numpy(idx)), (False, planes.to(torch.uint8))):
        v = SegmentationValidator(overlap_mask=overlap, max_gt=4)
        bits, area = v.pack_masks(dict(labels, masks=masks), 3, (160, 160), dev)
        torch.cuda.synchronize()
        assert bits.shape == (3, 4, 800) and area.shape == (3, 4)
        got = V.unpack_bits(_u32(bits), 25600)
        k0 = 0
        for i, k in enumerate(n):
            assert np.array_equal(got[i, :k], want[k0:k0 + k].reshape(k, 25600)), (overlap, i)
            assert not got[i, k:].any() and np.array_equal(area[i].cpu().numpy()[:k], want[k0:k0 + k].reshape(k, 25600).sum(-1))
            k0 += k


# ---- 2. the mask bits against upa_process_mask -------------------------------------------------------------------------------------

def _boxes(n, H, W, key):
    """Boxes in network-input pixels (4 px per proto pixel): random ones, then the edge cases."""
    u = P.hash_uniform(key, 4 * n).reshape(n, 4)
    x1, y1 = u[:, 0] * W * 0.8, u[:, 1] * H * 0.8
    b = np.stack([x1, y1, x1 + 4 + u[:, 2] * W * 0.5, y1 + 4 + u[:, 3] * H * 0.5], 1).astype(np.float32)
    edge = [[W + 8, H + 8, W + 40, H + 40],      # wholly outside the map
            [-30.5, -12.25, W * 0.5, H * 0.5],   # negative corners
            [W * 0.7, 4, W * 0.2, H - 4],        # x2 < x1: empty
            [-5, -5, W + 5, H + 5],              # covers the whole map
            [8, 12, 12, 16],                     # one proto pixel
            [4, 8, W - 8, H - 4],                # edges exactly on integer proto coordinates
            [6, 6, 6, 6]]                        # zero area
    b[:len(edge)] = np.array(edge, np.float32)[:n]
    return b


CASES = [(torch.float32, 32, (8, 8), 0), (torch.float32, 8, (20, 28), 0), (torch.bfloat16, 32, (20, 28), 0), (torch.bfloat16, 8, (8, 8), 0),
         (torch.float32, 32, (40, 40), 48), (torch.bfloat16, 32, (40, 40), 48), (torch.bfloat16, 32, (160, 160), 0),
         (torch.float32, 32, (160, 160), 0)]


@pytest.mark.parametrize("dtype,nm,hw,ldp", CASES, ids=[f"{str(c[0])[6:]}-nm{c[1]}-{c[2][0]}x{c[2][1]}" + ("-slice" if c[3] else "") for c in CASES])
@KC.stop_after_fault
def test_mask_bits_equal_process_mask(dtype, nm, hw, ldp):
    from ultralytics_pro_amd.utils import metrics as M
    from ultralytics_pro_amd.utils import ops
    dev = _dev()
    mh, mw = hw
    H, W = 4 * mh, 4 * mw
    b, max_det = 3, 64
    counts = [0, 37, min(300, max_det)]
    words = V.words_of(mh * mw)
    key = f"segval:bits:{nm}:{hw}"
    buf = torch.full((b, mh, mw, ldp or nm), 9.0, dtype=dtype, device=dev)  # a channel slice of a wider buffer when ldp is given
    buf[..., :nm] = P.uniform(key + ":p", (b, mh, mw, nm), -1.0, 1.0).to(dev).to(dtype)
    protos = buf.permute(0, 3, 1, 2)[:, :nm]
    rows = torch.full((b, max_det, 6 + nm), float("nan"))
    for i in range(b):
        rows[i, :, :4] = torch.from_numpy(_boxes(max_det, H, W, f"{key}:b{i}"))
        rows[i, :, 4] = 0.5
        rows[i, :, 5] = torch.arange(max_det) % 3
        rows[i, :, 6:] = P.uniform(f"{key}:c{i}", (max_det, nm), -1.0, 1.0)
    rows = rows.to(dev)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    # upa_process_mask, mode 0, out = (mh, mw): ragged rows
    total_rows = sum(counts)
    ref = torch.full((total_rows, mh, mw), 0xFF, dtype=torch.uint8, device=dev)
    nonempty = torch.empty((total_rows,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    ops._launch_process_mask(protos, rows[..., 6:], 6 + nm, rows, 6 + nm, max_det, cnt, (mh, mw), False, (mw / W, mh / H), (0, 0, mh, mw),
                             ref, nonempty, total_rows, total)
    gt_cls = torch.zeros((b, 2), device=dev)
    gt_bits = torch.zeros((b, 2, words), dtype=torch.int32, device=dev)
    gt_area = torch.zeros((b, 2), dtype=torch.int32, device=dev)
    ngt = torch.zeros((b,), dtype=torch.int32, device=dev)

    def once():
        pb = torch.full((b, max_det, words), -1, dtype=torch.int32, device=dev)
        pa = torch.full((b, max_det), -1, dtype=torch.int32, device=dev)
        tp = torch.full((b, max_det, 10), 0xFF, dtype=torch.uint8, device=dev)
        M.match_masks_batched(protos, rows, cnt, (H, W), gt_cls, gt_bits, gt_area, ngt, out=tp, pred_bits=pb, pred_area=pa)
        return pb, pa, tp

    pb, pa, tp = KC.twice(once)
    assert int(total.item()) == total_rows
    refm = ref.cpu().numpy().astype(bool).reshape(total_rows, -1)
    assert refm.any() and not refm.all()
    got = V.unpack_bits(_u32(pb), mh * mw)
    base = 0
    for i, n in enumerate(counts):
        assert np.array_equal(got[i, :n], refm[base:base + n]), f"image {i}: mask bits differ from upa_process_mask"
        assert np.array_equal(pa[i, :n].cpu().numpy(), refm[base:base + n].sum(-1))
        assert not _u32(pb)[i, n:].any() and not pa[i, n:].any()  # rows past counts: zero words, zero area
        base += n
    if (mh * mw) % 32:
        assert not (_u32(pb)[..., -1] >> ((mh * mw) % 32)).any()
    assert not tp.any()  # no labels: no true positive, every byte written
    assert bool((buf[..., nm:] == 9.0).all())


# ---- 3. IoU and TP against the checker and the goldens ---------------------------------------------------------------------------

def _run_bits(cases, G, hw, max_det, max_gt, garbage=False):
    """A batch of golden cases (one image each) through upa_segment_match_bits -> (iou_out (B, max_det, max_gt), tp (B, max_det, 10))."""
    from ultralytics_pro_amd.utils import metrics as M
    dev = _dev()
    npix = hw[0] * hw[1]
    words = V.words_of(npix)
    b = len(cases)
    db = np.full((b, max_det, words), 0xFFFFFFFF, np.uint32)   # rows past counts: garbage the kernel must not read into a result
    da = np.full((b, max_det), 12345, np.int32)
    det = np.full((b, max_det, 6), np.nan, np.float32)
    gb = np.full((b, max_gt, words), 0xFFFFFFFF, np.uint32)
    ga = np.full((b, max_gt), 777, np.int32)
    gc = np.full((b, max_gt), 1.0, np.float32)
    cnt, ngt = [], []
    for i, name in enumerate(cases):
        p, g = G[f"{name}_pred_bits"], G[f"{name}_gt_bits"]
        n, m = p.shape[0], g.shape[0]
        db[i, :n], da[i, :n] = p, V.unpack_bits(p, npix).sum(-1)
        det[i, :n, 5] = G[f"{name}_pred_cls"]
        gb[i, :m], ga[i, :m], gc[i, :m] = g, V.unpack_bits(g, npix).sum(-1), G[f"{name}_gt_cls"]
        cnt.append(n); ngt.append(m)
    if garbage and npix % 32:  # padding bits of the label AND prediction rows set: no count may change
        gb[..., -1] |= np.uint32(0xFFFFFFFF) << np.uint32(npix % 32)
        db[..., -1] |= np.uint32(0xFFFFFFFF) << np.uint32(npix % 32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    args = (_i32(db).to(dev), t(da), t(det), torch.tensor(cnt, dtype=torch.int32, device=dev), hw, t(gc), _i32(gb).to(dev), t(ga),
            torch.tensor(ngt, dtype=torch.int32, device=dev))

    def once():
        iou = torch.full((b, max_det, max_gt), float("nan"), device=dev)
        tp = M.match_mask_bits_batched(*args, iou_out=iou)
        return iou, tp

    iou, tp = KC.twice(once)
    return iou.cpu().numpy(), tp.cpu().numpy(), cnt, ngt


def _check_bits(cases, G, iou, tp, cnt, ngt):
    for i, name in enumerate(cases):
        n, m = cnt[i], ngt[i]
        same = G[f"{name}_gt_cls"][:, None] == G[f"{name}_pred_cls"][None]
        assert np.array_equal(iou[i, :n, :m], (G[f"{name}_iou"] * same).T), f"{name}: IoU"   # class-unequal pairs are written as 0
        assert np.array_equal(tp[i, :n].astype(bool), G[f"{name}_tp"]), f"{name}: TP"
        assert not tp[i, n:].any() and not iou[i, n:].any() and not iou[i, :, m:].any(), f"{name}: rows past counts / columns past ngt"
    assert not np.isnan(iou).any() and tp.max(initial=0) <= 1


@pytest.mark.parametrize("garbage", [False, True], ids=["clean", "padding-bits-set"])
@KC.stop_after_fault
def test_iou_and_tp_equal_reference_ragged_batch(OPS, garbage):
    """The four (20, 28) cases as ONE batch: counts (0, 37, 37, 300) and label counts (5, 5, 70, 1) side by side, 560 pixels = a half
    last word.  Classes 7 (labels only) and 9 (predictions only) are in the cases."""
    cases = ["n0_m5", "n37_m5", "n37_m70", "n300_m1"]
    assert 7.0 in OPS["n37_m70_gt_cls"] and 9.0 in OPS["n37_m5_pred_cls"] and 7.0 not in OPS["n37_m70_pred_cls"]
    iou, tp, cnt, ngt = _run_bits(cases, OPS, (20, 28), 300, 70, garbage)
    _check_bits(cases, OPS, iou, tp, cnt, ngt)
    assert tp.sum() > 15


@pytest.mark.parametrize("name", ["n1_m1", "n5_m0", "n300_m64"])
@KC.stop_after_fault
def test_iou_and_tp_equal_reference_single(OPS, name):
    hw = tuple(int(v) for v in OPS[f"{name}_hw"])
    n, m = OPS[f"{name}_pred_bits"].shape[0], OPS[f"{name}_gt_bits"].shape[0]
    iou, tp, cnt, ngt = _run_bits([name], OPS, hw, max(n, 1), max(m, 1))
    _check_bits([name], OPS, iou, tp, cnt, ngt)


@KC.stop_after_fault
def test_tp_on_the_references_own_masks(MAP):
    """Image 0 of the mask-mAP set, the reference's stored 160 x 160 masks: tp_m and the IoU matrix equal the reference's, through
    the public single-image form as well."""
    from ultralytics_pro_amd.utils import metrics as M
    dev = _dev()
    pb = MAP["pred_bits0"]
    k = pb.shape[0]
    det, gcls, gbits = MAP["det0"][:k], MAP["gt_cls0"], MAP["gt_bits0"]
    G = {"x_pred_bits": pb, "x_pred_cls": det[:, 5], "x_gt_bits": gbits, "x_gt_cls": gcls, "x_iou": MAP["mask_iou0"][:, :k],
         "x_tp": V.process_batch_masks(V.unpack_bits(pb, 25600), det[:, 5], V.unpack_bits(gbits, 25600), gcls)[1]}
    if k == MAP["det0"].shape[0]:
        assert np.array_equal(G["x_tp"], MAP["tp_m0"])
        G["x_tp"] = MAP["tp_m0"]
    iou, tp, cnt, ngt = _run_bits(["x"], G, (160, 160), 300, 64)
    _check_bits(["x"], G, iou, tp, cnt, ngt)
    assert tp.sum() > 0
    pm = torch.from_numpy(V.unpack_bits(pb, 25600).reshape(k, 160, 160)).to(dev)
    gm = torch.from_numpy(V.unpack_bits(gbits, 25600).reshape(-1, 160, 160)).to(dev)
    got = M.process_batch_masks(pm, torch.from_numpy(det[:, 5]).to(dev), gm.float(), torch.from_numpy(gcls).to(dev))
    assert np.array_equal(got, G["x_tp"])


# ---- 4. public functions ------------------------------------------------------------------------------------------------------------

@KC.stop_after_fault
def test_mask_iou_public(OPS, MAP):
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.utils import metrics as M
    dev = _dev()
    for name in ("n37_m5", "n300_m64", "n37_m70"):
        hw = OPS[f"{name}_hw"]
        npix = int(hw[0] * hw[1])
        p, g = V.unpack_bits(OPS[f"{name}_pred_bits"], npix), V.unpack_bits(OPS[f"{name}_gt_bits"], npix)
        for cast in (lambda a: torch.from_numpy(a.astype(np.float32)), lambda a: torch.from_numpy(a.astype(np.uint8))):
            out = KC.twice(lambda: (M.mask_iou(cast(g).to(dev), cast(p).to(dev)),))[0]
            assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), OPS[f"{name}_iou"]), name
    k = MAP["pred_bits0"].shape[0]
    out = M.mask_iou(torch.from_numpy(V.unpack_bits(MAP["gt_bits0"], 25600)).float().to(dev),
                     torch.from_numpy(V.unpack_bits(MAP["pred_bits0"], 25600).astype(np.uint8)).to(dev))
    assert np.array_equal(out.cpu().numpy(), MAP["mask_iou0"][:, :k])
    a = torch.zeros((3, 64), device=dev)
    assert M.mask_iou(a[:0], a).shape == (0, 3) and M.mask_iou(a, a[:0]).shape == (3, 0)
    assert float(M.mask_iou(a, a).abs().sum()) == 0.0  # empty against empty: 0, not NaN
    with pytest.raises(UpaError):
        M.mask_iou(torch.zeros(2, 64), torch.zeros(3, 64))
    with pytest.raises(UpaError):
        M.process_batch_masks(torch.zeros(2, 8, 8), torch.zeros(2), torch.zeros(1, 8, 8), torch.zeros(1))
    assert M.process_batch_masks(torch.zeros(0, 8, 8), torch.zeros(0), torch.zeros(1, 8, 8), torch.zeros(1)).shape == (0, 10)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

@KC.stop_after_fault
def test_refusals_leave_every_buffer_untouched():
    from ultralytics_pro_amd import _lib as L
    dev = _dev()
    mh = mw = 8
    words, max_det, b = 2, 4, 1
    thr = np.ascontiguousarray(V.IOUV)

    def call(nm=32, ldp=None, dtype=L.UPA_F32, max_gt=4, null=None, ws_short=False):
        ldp = ldp or nm
        protos = torch.zeros((b, mh, mw, ldp), device=dev)
        rows = torch.zeros((b, max_det, 6 + nm), device=dev)
        cnt = torch.full((b,), max_det, dtype=torch.int32, device=dev)
        gcls = torch.zeros((b, max_gt), device=dev)
        gb = torch.zeros((b, max_gt, words), dtype=torch.int32, device=dev)
        ga = torch.zeros((b, max_gt), dtype=torch.int32, device=dev)
        ngt = torch.full((b,), min(max_gt, 4), dtype=torch.int32, device=dev)
        tp = torch.full((b, max_det, 10), 0xFF, dtype=torch.uint8, device=dev)
        pb = torch.full((b, max_det, words), -1, dtype=torch.int32, device=dev)
        pa = torch.full((b, max_det), -1, dtype=torch.int32, device=dev)
        iou = torch.full((b, max_det, max_gt), float("nan"), device=dev)
        ws = torch.full((b * max_det,), -1, dtype=torch.int64, device=dev)
        ptr = dict(protos=protos.data_ptr(), rows=rows.data_ptr(), counts=cnt.data_ptr(), gt_cls=gcls.data_ptr(), gt_bits=gb.data_ptr(),
                   gt_area=ga.data_ptr(), ngt=ngt.data_ptr(), thr=thr.ctypes.data, tp=tp.data_ptr(), ws=ws.data_ptr())
        if null:
            ptr[null] = None
        rc = L.lib().upa_segment_match(ptr["protos"], b, mh, mw, nm, ldp, dtype, ptr["rows"], 6 + nm, max_det, ptr["counts"], 0.25, 0.25,
                                       ptr["gt_cls"], 1, ptr["gt_bits"], ptr["gt_area"], ptr["ngt"], max_gt, ptr["thr"], 10, ptr["tp"],
                                       pb.data_ptr(), pa.data_ptr(), iou.data_ptr(), ptr["ws"], 0 if ws_short else b * max_det * 8,
                                       L.current_stream(dev))
        torch.cuda.synchronize()
        untouched = (bool((tp == 0xFF).all()) and bool((pb == -1).all()) and bool((pa == -1).all()) and bool(torch.isnan(iou).all())
                     and bool((ws == -1).all()))
        return rc, untouched

    EINVAL, EUNSUPPORTED = -1, L.UPA_EUNSUPPORTED
    assert call() == (0, False)                                   # the accepted form writes
    assert call(nm=136) == (EUNSUPPORTED, True)                   # nm > 128
    assert call(dtype=2) == (EUNSUPPORTED, True)                  # neither f32 nor bf16
    assert call(nm=6, ldp=8) == (EINVAL, True)                    # nm not a 16-byte group
    assert call(nm=32, ldp=34) == (EINVAL, True)                  # ldp not a 16-byte group
    assert call(max_gt=4096) == (EINVAL, True)                    # 4096 x 10 x 4 B claim table > LDS
    assert call(ws_short=True) == (EINVAL, True)
    for name in ("protos", "rows", "counts", "gt_cls", "gt_bits", "gt_area", "ngt", "thr", "tp", "ws"):
        assert call(null=name) == (EINVAL, True), name
    assert b"null" in L.lib().upa_last_error()


# ---- 6. the validate path ---------------------------------------------------------------------------------------------------------

def _labels(MAP, dev, max_gt=64):
    gt = torch.zeros(4, max_gt, 5)
    bits = np.zeros((4, max_gt, 800), np.uint32)
    ngt = []
    for i in range(4):
        gc, gb = torch.from_numpy(MAP[f"gt_cls{i}"]), torch.from_numpy(MAP[f"gt_boxes{i}"])
        m = gc.shape[0]
        gt[i, :m, 0], gt[i, :m, 1:] = gc, gb
        bits[i, :m] = MAP[f"gt_bits{i}"]
        ngt.append(m)
    area = V.unpack_bits(bits, 25600).sum(-1).astype(np.int32)
    return gt.to(dev), torch.tensor(ngt, dtype=torch.int32, device=dev), _i32(bits).to(dev), torch.from_numpy(area).to(dev)


def _seg_model(dev):
    from ultralytics_pro_amd.nn.tasks import SegmentationModel
    m = SegmentationModel("yolov8n-seg.yaml")
    P.apply_procedural_weights(m, family="yolov8n-seg")
    return m.to(dev).eval()


@KC.stop_after_fault
def test_segmentation_validator_matches_reference_map(MAP):
    """SegmentationModel("yolov8n-seg.yaml") in f32 on the four synthetic images, as one batch and as two batches of two: box and
    mask means within the project's 5e-3 of the reference's (the gate of tests/test_metrics.py).  The product's detections differ
    from the reference's by <= 1e-3 px and its mask logits in the last bits, so only a pair sitting on an IoU threshold - or a pixel
    on the zero crossing that moves such a pair - can flip: printed beside the fixture's near_threshold count."""
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.validator import DetectionValidator, SegmentationValidator
    dev = _dev()
    m = _seg_model(dev)
    with pytest.raises(UpaError):
        DetectionValidator(m)
    x = P.synthetic_images(4).to(dev)
    gt, ngt, gbits, garea = _labels(MAP, dev)
    # the packing path gives the same label rows as the stored ones (160 x 160 planes, no resize)
    planes = torch.from_numpy(np.concatenate([V.unpack_bits(MAP[f"gt_bits{i}"], 25600).reshape(-1, 160, 160) for i in range(4)], 0))
    lab = dict(batch_idx=torch.cat([torch.full((int(k),), i) for i, k in enumerate(ngt.tolist())]), masks=planes.to(torch.uint8))
    pb, pa = SegmentationValidator(overlap_mask=False).pack_masks(lab, 4, (160, 160), dev)
    assert torch.equal(pb, gbits) and torch.equal(pa, garea)
    ref_tpm = np.concatenate([MAP[f"tp_m{i}"] for i in range(4)], 0)
    for split in ((0, 4),), ((0, 2), (2, 4)):
        v = SegmentationValidator(m)
        with torch.no_grad():
            for a, b in split:
                v.update(m(x[a:b].contiguous()), gt[a:b].contiguous(), ngt[a:b].contiguous(), gbits[a:b].contiguous(), garea[a:b].contiguous())
        st = v.get_stats()
        box, seg = np.array(st["mean"]), np.array(st["seg"]["mean"])
        flipped = int((st["tp_m"] != ref_tpm).sum()) if st["tp_m"].shape == ref_tpm.shape else -1
        print(f"validator {split}: box {box} (reference {MAP['mean']}), mask {seg} (reference {MAP['seg_mean']}); "
              f"tp_m entries that differ from the reference's: {flipped} (-1: row counts differ); near_threshold {int(MAP['near_threshold'])}")
        assert np.abs(box - MAP["mean"]).max() <= 5e-3
        assert np.abs(seg - MAP["seg_mean"]).max() <= 5e-3
        assert st["tp"].shape == st["tp_m"].shape and st["tp_m"].any()


# ---- 7. graph ---------------------------------------------------------------------------------------------------------------------

@KC.stop_after_fault
def test_update_step_graph_replay_equals_eager(MAP):
    from ultralytics_pro_amd.engine.validator import SegmentationValidator
    dev = _dev()
    m = _seg_model(dev)
    x = P.synthetic_images(2).to(dev).contiguous()
    gt, ngt, gbits, garea = (t[:2].contiguous() for t in _labels(MAP, dev))
    v = SegmentationValidator(m)
    post = lambda o: v.update(o, gt, ngt, gbits, garea, key="segval_replay", record=False)  # noqa: E731
    with torch.no_grad():
        e = post(m(x))
        torch.cuda.synchronize()
        eager = [t.clone() for t in e]
        run = m.compile(x, post=post)
        r1 = [t.clone() for t in run()]
        r2 = run()
    torch.cuda.synchronize()
    assert int(eager[1].sum()) > 0 and bool(eager[3].any())
    for a, b_, c in zip(eager, r1, r2):
        assert torch.equal(a, b_) and torch.equal(a, c)
    v.add_batch_stats(*r2[:3], gt, ngt, r2[3])
    assert v.get_stats()["tp_m"].shape[0] == int(eager[1].sum())
