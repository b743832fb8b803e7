"""-m gpu: the post-processing kernels against the exact reference tests/postprocess_ref.py on built scenes - the NMS kernels of
csrc/nms.hip (`nms_candidates`, `nms_hist`, `nms_emit`, `nms_sort`, `nms_greedy`) through `nms_raw`, and the box side of validation in
csrc/metrics.hip (`upa_match_predictions`, `upa_box_iou`, `upa_scale_boxes`).

Every NMS and matching comparison is bit-exact on the fixed-shape outputs: rows, counts, keep indices, the zero rows past counts[b] and
keep == -1 there.  The scenes are decidable (tests/test_postprocess_ref.py asserts it on the CPU and pins the reference against
oracle/nms.py and the reference goldens), so any difference is the kernel's.  What each structural scene guards in nms_greedy_kernel:
chains - the fixed point `kn == k` of the suppression columns; alive7/8/9 - `by_cols` at GREEDY_ROWS_MIN; slices - the phase 1 loop
`for (k = wave; k < kept; k += GREEDY_NW)`; cut_* and iso1100 - `room` and MAX_DET_CAP; stage* - the stage loop's `li` / `stage_n`;
maxnms_* - the radix select of nms_sort_kernel; match* - the rounds of 256 of match_predictions_kernel around `match_claim_round`."""

import numpy as np
import pytest
import torch

from tests import postprocess_ref as PR
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

NAMES = [s.name for s in PR.scenes()]
STAGED = [n for n in NAMES if n.endswith("-ml") and (n.startswith("chain") or n.startswith("tie_"))]


def _dev():
    from tests.hip_utils import DEV
    return DEV


def _poison(*shapes_dtypes):
    """Best effort against stale results: blocks of the sizes the call is about to allocate, filled with 0xFF bytes and freed."""
    for shape, dtype in shapes_dtypes:
        t = torch.empty(shape, dtype=dtype, device=_dev())
        t.view(torch.uint8).fill_(0xFF)
        del t


def _nms(s, hot=False, pred=None):
    from ultralytics_pro_amd.utils.nms import nms_raw
    p = torch.from_numpy(s.pred if pred is None else pred).to(_dev())
    if hot:
        keys = PR.best_keys(s.pred, s.nc)
        unwritten = (s.pred[:, 4:4 + s.nc].max(1) == 0) & (np.arange(s.pred.shape[2])[None] % 2 == 1)
        keys[unwritten] = -1  # anchors no class launch wrote: the buffer's initial word, score 0
        p._upa_hot = torch.from_numpy(keys).to(_dev())
    b, md = s.pred.shape[0], s.kw.get("max_det", 300)
    _poison(((b, md, 6), torch.float32), ((b,), torch.int32), ((b, md), torch.int32))
    out, counts, keep = nms_raw(p, **s.kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), counts.cpu().numpy(), keep.cpu().numpy()


def _assert_nms(got, s, what):
    rows, counts, keep = s.fixed()
    assert np.array_equal(got[1], counts), (s.name, what, got[1], counts)
    bad = np.nonzero((got[0].view(np.uint32) != rows.view(np.uint32)).any(2))
    assert bad[0].size == 0, (s.name, what, "first differing row", bad[0][0], bad[1][0], got[0][bad[0][0], bad[1][0]], rows[bad[0][0], bad[1][0]])
    assert np.array_equal(got[2], keep), (s.name, what)


@pytest.mark.parametrize("name", NAMES)
@KC.stop_after_fault
def test_nms_scene_bit_exact(name):
    """Rows, counts, keep indices and the fixed-shape tail of every scene; single-label scenes again through the best-class-key entry
    (`upa_nms_batched_hot`: the sort kernel compacts the candidates itself), bit for bit the plain path."""
    s = PR.scene(name)
    plain = _nms(s)
    _assert_nms(plain, s, "plain")
    again = _nms(s)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again)), "two runs differ"
    if s.single_label:
        _assert_nms(_nms(s, hot=True), s, "hot")


@KC.stop_after_fault
def test_hot_entry_reads_the_keys_not_the_scores():
    """With the keys attached, single-label NMS takes score and class from them: the class rows may hold anything (keys-only Detect)."""
    for name in ("chain200_from60-sl", "tie_classes_nc17-sl", "stage1025-sl", "classes_filter-sl"):
        s = PR.scene(name)
        junk = s.pred.copy()
        junk[:, 4:] = 0.99
        _assert_nms(_nms(s, hot=True, pred=junk), s, "hot, junk scores")


@pytest.mark.parametrize("staging", [{"nms_stages": 1}, {"nms_stages": 2}, {"nms_first_prefix": 256}], ids=["all_keys", "radix_select", "prefix_256"])
@KC.stop_after_fault
def test_nms_staging_does_not_change_results(staging):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    assert "chain200_from60_staged-ml" in STAGED and "tie_classes_staged-ml" in STAGED
    for name in STAGED:
        s = PR.scene(name)
        with R.use_opts(L.Opts(**staging)):
            _assert_nms(_nms(s), s, staging)


@KC.stop_after_fault
def test_nms_wrapper_and_max_det_cap():
    """The list-returning wrapper on a ragged batch, and max_det above the kept-list capacity (1024) refused."""
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.utils.nms import non_max_suppression, nms_raw
    for name in ("shape_A257_B3-sl", "shape_A65_B3-ml"):
        s = PR.scene(name)
        out, keep = non_max_suppression(torch.from_numpy(s.pred).to(_dev()), return_idxs=True, **s.kw)
        for (rows, k, _, _), o, ki in zip(s.ref(), out, keep):
            assert np.array_equal(o.cpu().numpy(), rows) and np.array_equal(ki.cpu().numpy(), k)
    s = PR.scene("iso1100_maxdet1024")
    with pytest.raises(L.UpaError):
        nms_raw(torch.from_numpy(s.pred).to(_dev()), **dict(s.kw, max_det=1025))
    torch.cuda.synchronize()


# ---- box matching -------------------------------------------------------------------------------------------------------------------


def _match(m):
    from ultralytics_pro_amd.utils import metrics as pmet
    dev = _dev()
    det, gt = torch.from_numpy(m.det).to(dev), torch.from_numpy(m.gt).to(dev)
    counts, ngt = torch.from_numpy(m.counts).to(dev), torch.from_numpy(m.ngt).to(dev)
    outs = []
    for _ in range(2):
        tp = torch.full((m.det.shape[0], m.det.shape[1], len(m.iouv)), 0xFF, dtype=torch.uint8, device=dev)
        pmet.match_predictions_batched(det, counts, gt, ngt, iouv=m.iouv, out=tp)
        torch.cuda.synchronize()
        outs.append(tp.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "two runs differ"
    return outs[0]


@pytest.mark.parametrize("max_det", [300, 600])
@KC.stop_after_fault
def test_match_predictions_bit_exact(max_det):
    """Contests over one label (also split across the rounds of 256 detections), IoU on a threshold and one ulp below, class mismatch,
    ragged B = 3 with ngt = 0 and counts = 0, counts / ngt above the buffers (clamped), zero rows at and past counts[b]."""
    for m in (PR.match_scene(max_det), PR.match_scene(max_det, True), PR.match_scene_clamped(max_det)):
        got, ref = _match(m), m.ref()
        bad = np.nonzero((got != ref).any(2))
        assert bad[0].size == 0, (m.name, "first differing row", bad[0][0], bad[1][0], got[bad[0][0], bad[1][0]], ref[bad[0][0], bad[1][0]])


@KC.stop_after_fault
def test_match_predictions_refusals():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.utils import metrics as pmet
    dev = _dev()
    m = PR.match_scene(300)
    det, counts = torch.from_numpy(m.det).to(dev), torch.from_numpy(m.counts).to(dev)
    gt, ngt = torch.from_numpy(m.gt).to(dev), torch.from_numpy(m.ngt).to(dev)
    with pytest.raises(L.UpaError):
        pmet.match_predictions_batched(det, counts, gt, ngt, iouv=m.iouv[:9])
    big = torch.zeros((3, 4100, 5), device=dev)  # 4100 labels x 10 thresholds x 4 bytes: over the LDS table
    with pytest.raises(L.UpaError):
        pmet.match_predictions_batched(det, counts, big, ngt)
    torch.cuda.synchronize()


# ---- box_iou, scale_boxes -----------------------------------------------------------------------------------------------------------


def _boxes(rng, n):
    """n xyxy boxes: a third on an integer grid, a third arbitrary f32, a third of zero area (w = 0, h = 0 or both)."""
    xy = rng.uniform(0, 600, (n, 2))
    wh = rng.uniform(1, 120, (n, 2))
    b = np.concatenate([xy, xy + wh], 1)
    b[0::3] = np.round(b[0::3])
    z = np.arange(n) % 3 == 2
    b[z, 2] = np.where(np.arange(n)[z] % 2 == 0, b[z, 0], b[z, 2])
    b[z, 3] = np.where(np.arange(n)[z] % 4 < 2, b[z, 3], b[z, 1])
    b[z & (np.arange(n) % 5 == 0), 2:] = b[z & (np.arange(n) % 5 == 0), :2]
    return b.astype(PR.F32)


@pytest.mark.parametrize("nm", [(15, 17), (16, 16), (1, 257), (257, 1), (0, 5)], ids=lambda v: f"{v[0]}x{v[1]}")
@KC.stop_after_fault
def test_box_iou_bit_exact(nm):
    """N M = 255, 256, 257 (the 256-thread block edge) and an empty side: bit-equal to the f32 restatement of utils/metrics.py:54-74, and as
    close to float64 as that restatement itself is on these inputs (the bound is measured, not chosen)."""
    from ultralytics_pro_amd.utils import metrics as pmet
    n, m = nm
    rng = np.random.default_rng(1000 * n + m)
    b1, b2 = _boxes(rng, n), _boxes(rng, m)
    if n and m:
        b2[-1] = b1[0]  # IoU 1 (up to eps)
    if n > 1 and m > 1:
        b1[-1] = b2[0] = (7, 9, 7, 9)  # two zero-area boxes on one point: 0 / eps = 0
    got = pmet.box_iou(torch.from_numpy(b1).to(_dev()), torch.from_numpy(b2).to(_dev()))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    r32, r64 = PR.box_iou_ref(b1, b2, dtype=PR.F32), PR.box_iou_ref(b1, b2, dtype=np.float64)
    assert got.shape == (n, m) and r32.dtype == PR.F32
    if not (n and m):
        return
    assert (got[-1, 0] == 0 or min(n, m) == 1) and np.isfinite(got).all() and got.max() > 0.99
    assert np.array_equal(got.view(np.uint32), r32.view(np.uint32))
    nz = r64 != 0
    bound = float((np.abs(r32.astype(np.float64) - r64)[nz] / r64[nz]).max())
    worst = float((np.abs(got.astype(np.float64) - r64)[nz] / r64[nz]).max())
    print(f"box_iou {n}x{m}: f32 restatement vs f64 worst relative difference {bound:.3e} ({bound / 2 ** -24:.2f} half-ulps), kernel {worst:.3e}")
    assert worst <= bound and (got[~nz] == 0).all()


@pytest.mark.parametrize("stride", [6, 38])
@pytest.mark.parametrize("padding", [True, False])
@KC.stop_after_fault
def test_scale_boxes_bit_exact(stride, padding):
    """Row strides 6 (detections) and 38 (detections + 32 mask coefficients), with and without the padding step, boxes that clip at all
    four borders, more rows than one block: columns 0-3 bit-equal to the f32 restatement of utils/ops.py:102-178, the others untouched."""
    from ultralytics_pro_amd.utils.ops import scale_boxes
    rng = np.random.default_rng(stride + int(padding))
    rows = rng.uniform(-3, 3, (300, stride)).astype(PR.F32)
    rows[:, :4] = _boxes(rng, 300)
    rows[0, :4], rows[1, :4] = (-50, -40, 700, 690), (-1, 100, 5, 700)  # left / top / right / bottom
    rows[2, :4], rows[3, :4] = (630, -3, 900, 50), (100, 600, 200, 900)
    for img1, img0, rp in (((640, 640), (1080, 810), None), ((384, 640), (720, 1280), None), ((640, 640), (500, 375), ((1.28,), (80.0, 0.0)))):
        got = scale_boxes(img1, torch.from_numpy(rows.copy()).to(_dev()), img0, ratio_pad=rp, padding=padding)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        ref = PR.scale_boxes_ref(img1, rows, img0, ratio_pad=rp, padding=padding, dtype=PR.F32)
        assert ref.dtype == PR.F32
        assert np.array_equal(got[:, :4].view(np.uint32), ref[:, :4].view(np.uint32)), (img1, img0, rp)
        assert np.array_equal(got[:, 4:].view(np.uint32), rows[:, 4:].view(np.uint32))
        assert (got[:4, :4] == 0).any() and (got[:4, [0, 2]] == img0[1]).any() and (got[:4, [1, 3]] == img0[0]).any()
        r64 = PR.scale_boxes_ref(img1, rows, img0, ratio_pad=rp, padding=padding, dtype=np.float64)
        assert np.abs(got[:, :4] - r64[:, :4]).max() <= 2 ** -22 * 1280  # the rounded gain, the subtraction and the division: under four half-ulps of values up to 1280
